/* Stand-in for <jack/types.h>: the four type names the compiled reference voice asks for.  Declarations only. */
#pragma once
#include <stdint.h>
typedef uint32_t jack_nframes_t;
typedef uint64_t jack_time_t;
typedef float jack_default_audio_sample_t;
typedef struct _jack_position jack_position_t;
