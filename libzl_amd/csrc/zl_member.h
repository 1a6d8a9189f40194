// zl_member.h -- what an engine group (zl_group.cpp) may do to its member engines beyond the C-ABI; defined in zl_engine.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../include/zlhip.h"
#include "zl_host.h"
#include "zl_types.h"

// the member's control plane, after the voices that ended on the device have freed their slots (*rc: ZLHIP_OK or the error)
ZlHostControl *zl_member_control(zlhip_engine *e, int *rc);
hipStream_t zl_member_stream(const zlhip_engine *e);               // the member's own stream: its render kernels run there
float *zl_member_last_bus(const zlhip_engine *e);                  // the bus buffer the last zlhip_render_batch wrote
ZlBlockLevels *zl_member_levels(const zlhip_engine *e);            // the block levels zlhip_levels_tick / zlhip_block_peaks read
