// zl_engine_impl.h -- the engine's state and the helpers its host files share: zl_engine.cpp (the engine itself, where every helper
// declared here is defined) and zl_clip_calls.cpp (the clip services).  Private to csrc/: nothing else includes it, and an engine
// group goes through zl_member.h.  The helpers and their types have hidden visibility: what the library exports does not grow by them.
// Every HIP resource the engine owns is a member of an owning type (zl_owned.h) and goes back in its destructor, at `delete e`; a plain
// hipEvent_t / hipStream_t member only names one that another member owns ("alias").  The exception: the arena's later segments (zl_arena.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_arena.h"
#include "zl_host.h"
#include "zl_owned.h"
#include "zl_types.h"

struct ZlOnOnset; struct ZlTpResult; struct ZlPtResult; struct ZlLdSub; struct ZlLpResult; struct ZlKyResult; struct ZlXfSums; struct ZlLmRecord;     // (zl_onset.h, zl_tempo.h, zl_pitch.h, zl_loudness.h, zl_loop.h, zl_key.h, zl_xfade.h, zl_limit.h)

#pragma GCC visibility push(hidden)
// scratch[]: a call's records and staging (GrowBuf; grow_buf); an engine that never re-renders, asks for an overview or loads PCM has none
enum { ZB_ST_JOBS, ZB_ST_LIST, ZB_ST_OFFS,                    // re-render: a call's jobs, the jobs whose stretch runs, their seek offsets
       ZB_OV_REQ, ZB_OV_COLS,                                 // overviews: a call's request records and its columns [columns][4], with host twins
       ZB_PCM_STAGE, ZB_PCM_PIECES, ZB_PCM_PUB, ZB_PCM_VERDICTS,   // PCM: the staging buffer for the raw bytes, a call's piece and publish records, its verdict words
       ZB_RS_JOBS, ZB_RS_PUB, ZB_RS_VERDICTS,                // rate conversion: a call's job and publish records, its verdict words
       ZB_ON_REQ, ZB_ON_E, ZB_ON_N, ZB_ON_PS,                // transients: a call's request records (with a host twin), and per hop E, N and the windows' running maxima
       ZB_TP_REQ, ZB_TP_E, ZB_TP_W, ZB_TP_A, ZB_TP_STAT,      // tempo: a call's request records (the energy pass's and the tempo kernels', one host twin), per hop E and W, per lag A, per request the flux's statistics
       ZB_PT_REQ, ZB_PT_D, ZB_PT_STAT, ZB_PT_FRAME,           // pitch: a call's request records (with a host twin), per frame and lag d, per frame the diff kernel's statistics and the frame records
       ZB_LD_REQ,                                             // loudness: a call's request records (with a host twin)
       ZB_LP_REQ, ZB_LP_X, ZB_LP_E, ZB_LP_SHIFT, ZB_LP_ITEM, ZB_LP_COST,   // loop finder: a call's request records (with a host twin), the int16 strips, per candidate E, per request the shift, the item records, the cost matrix (small calls)
       ZB_KY_REQ, ZB_KY_BINS, ZB_KY_TABLE, ZB_KY_STAT, ZB_KY_ACC, ZB_KY_TOTAL,   // key: a call's request records, its bin tables and the paired cosine table (each with a host twin), per frame the gate's verdict, per frame and bin re and im, per bin the totals
       ZB_XF_JOBS, ZB_XF_WEIGHTS, ZB_XF_PUB, ZB_XF_VERDICTS,  // loop crossfade: a call's job records, its (a, b) pairs, its publish records, its verdict words
       ZB_ED_SCAN, ZB_ED_FOUND, ZB_ED_JOBS, ZB_ED_WEIGHTS, ZB_ED_PUB, ZB_ED_VERDICTS,   // clip edit: a call's scan records and their two words each, its job records, its fade weights, its publish records, its verdict words
       ZB_LM_SCAN, ZB_LM_TABLES, ZB_LM_REC, ZB_LM_JOBS, ZB_LM_WEIGHTS, ZB_LM_STATS, ZB_LM_PUB, ZB_LM_VERDICTS,   // peaks and limiter: a call's detecting records and the two filter tables (each with a host twin), the limiter's chunk records, its job records, its windows, its statistics, its publish records, its verdict words
       ZB_WP_JOBS, ZB_WP_REGIONS, ZB_WP_LIST, ZB_WP_OFFS, ZB_WP_PUB, ZB_WP_VERDICTS,   // warp: a call's job and region records, the regions whose seek runs, the seek offsets, its publish records, its verdict words
       ZB_COUNT };

// Stage times of a call (zlhip_set_profiling): events 0 .. N-1 recorded between the call's launches.  `on` is set by every call from the
// engine's switch; while it is off nothing is created, recorded or read, and the times stay those of the last profiled call.  An event
// is created by the first mark that needs it.
template <int N> struct ZlStageTimer {
    ZlEvent ev[N]; bool on = false;
    hipError_t mark(int i, hipStream_t s)
    {
        if (!on) return hipSuccess;
        if (!ev[i]) { const hipError_t r = ev[i].create(); if (r != hipSuccess) return r; }
        return hipEventRecord(ev[i], s);
    }
    hipError_t elapsed(int a, int b, float *ms) { return on ? hipEventElapsedTime(ms, ev[a], ev[b]) : hipSuccess; }   // after the call's wait
};
#pragma GCC visibility pop

struct zlhip_engine {
    zlhip_config cfg{};
    int V = 0;
    int device = 0;
    ZlStream stream;
    std::string err;
    char devname[256] = {0};

    // HBM
    ZlDev<float> arena;
    // the arena's allocator (zl_arena.h): the free extents of the first arena and of the further segments, allocated when a source does
    // not fit any more (clips are loaded freely; 288 GB of HBM).  A source in a segment is addressed like any other, by its float offset
    // from `arena` modulo 2^64, which the kernels' 64-bit address arithmetic wraps back.  A segment's handle is its device pointer.
    ZlArena arenaAlloc;
    // per sound slot, next to hc.sounds (what the slot plays) and hc.soundUsed: the original upload -- every re-render
    // (zlhip_sound_rerender) starts from it, as tracktion renders from the clip's source file -- and the render it plays instead while it has one
    struct SoundSlot {
        ZlSound orig{0, 0, 0, 0.0}; size_t floats = 0;   // the original upload, the floats it holds in the arena
        size_t renderFloats = 0;         // floats of the slot's rendered extent, 0 = it plays its original
        std::vector<int32_t> renderOffsets;   // the seek offsets of the slot's last render (zlhip_debug_rerender_offsets)
        std::vector<int32_t> warpOffsets;     // the seek offsets of the slot's last warp (zlhip_debug_warp_offsets)
    };
    std::vector<SoundSlot> soundSlots;
    GrowBuf scratch[ZB_COUNT];           // a call's records and staging (grow_buf)
    // the clip services' state (zl_clip_calls.cpp); each `timer` with the times of the last call made with profiling on (zlhip_debug_*_timings)
    struct Rerender { ZlStageTimer<3> timer; float seekMs = 0.0f, synthMs = 0.0f; } st;     // marks: before the seek, between the launches, after
    struct Overview { ZlStageTimer<2> timer; float ms = 0.0f; } ov;                         // marks: around the call's launches
    // transients (zlhip_sound_onsets; zl_onset.h)
    struct Onset {
        ZlMapped<int32_t> counts; ZlMapped<ZlOnOnset> out;          // a call's counts and onsets: the pick kernel writes what it found and nothing else crosses
        std::vector<std::pair<int32_t, int32_t>> last;              // per request of the last call: its first hop, its hops (zlhip_debug_onset_hops)
        ZlStageTimer<3> timer; float energyMs = 0.0f, restMs = 0.0f;
    } on;
    // tempo (zlhip_sound_tempo; zl_tempo.h)
    struct Tempo {
        ZlMapped<ZlTpResult> out;                                   // a call's integer records
        struct Last { int32_t hop_base, hops, acf_base, first_lag, nlags; };
        std::vector<Last> last;                                     // per request of the last call (zlhip_debug_tempo_acf)
        ZlStageTimer<5> timer; float energyMs = 0.0f, acfMs = 0.0f, restMs = 0.0f;
    } tp;
    // pitch (zlhip_sound_pitch; zl_pitch.h)
    struct Pitch {
        ZlMapped<ZlPtResult> out;                                   // a call's integer records
        struct Last { int64_t d_base; int32_t frame_base, frames, nd; };
        std::vector<Last> last;                                     // per request of the last call (zlhip_debug_pitch_frames / _diff)
        ZlStageTimer<3> timer; float diffMs = 0.0f, restMs = 0.0f;
    } pt;
    // loudness (zlhip_sound_loudness; zl_loudness.h)
    struct Loudness {
        ZlMapped<ZlLdSub> out;                                      // a call's sub-block records
        struct Last { int32_t item_base, items; };
        std::vector<Last> last;                                     // per request of the last call (zlhip_debug_loudness_subs)
        ZlStageTimer<2> timer; float kernelMs = 0.0f;
    } ld;
    // loop finder (zlhip_sound_loop; zl_loop.h)
    struct Loop {
        ZlMapped<ZlLpResult> out;                                   // a call's integer records
        struct Last { int64_t cost_base; int32_t item_base, items, ns, ne; };
        std::vector<Last> last;                                     // per request of the last call (zlhip_debug_loop_items / _costs)
        bool costs = false;                                         // the last call stored its cost matrix
        ZlStageTimer<4> timer; float pairsMs = 0.0f, restMs = 0.0f; // marks: before the prep, around the pairs kernel, behind the pick
    } lp;
    // key (zlhip_sound_key; zl_key.h)
    struct Key {
        ZlMapped<ZlKyResult> out;                                   // a call's integer records
        struct Last { int64_t acc_base; int32_t bin_base, nbins, frames; };
        std::vector<Last> last;                                     // per request of the last call (zlhip_debug_key_bins / _frame)
        ZlStageTimer<4> timer; float gateMs = 0.0f, correlateMs = 0.0f, foldMs = 0.0f;   // marks: around each of the three launches
    } ky;
    // loop crossfade (zlhip_sound_loop_crossfade; zl_xfade.h)
    struct Xfade {
        ZlMapped<ZlXfSums> sums;                                    // a call's measured sums, one record per applied request
        ZlStageTimer<4> timer; float measureMs = 0.0f, renderMs = 0.0f;   // marks: around the measuring launch, around the render and publish launches
    } xf;
    // clip edit (zlhip_sound_edit; zl_edit.h)
    struct Edit { ZlStageTimer<4> timer; float scanMs = 0.0f, renderMs = 0.0f; } ed;      // marks: around the scanning launch, around the render and publish launches
    // peaks and limiter (zlhip_sound_peak, zlhip_sound_limit; zl_limit.h)
    struct Limit {
        ZlMapped<ZlLmRecord> out;                                   // an analysis call's chunk records
        struct Last { int32_t rec_base, chunks; };
        std::vector<Last> last;                                     // per request of the last analysis call (zlhip_debug_peak_chunks)
        std::vector<float> tables;                                  // the two filter tables, made by the first call that asks for the true peak
        ZlStageTimer<2> peakTimer; float peakMs = 0.0f;             // marks: around the analysis launch
        ZlStageTimer<4> timer; float detectMs = 0.0f, renderMs = 0.0f;   // marks: around the detecting launch, around the render and publish launches
    } lm;
    // warp (zlhip_sound_warp; zl_warp.h)
    struct Warp { ZlStageTimer<3> timer; float seekMs = 0.0f, synthMs = 0.0f; } wp;       // marks: before the seek, between the launches, behind the publish
    // clips from raw PCM (zlhip_sound_upload_pcm; zl_decode.h)
    struct Pcm {
        std::vector<ZlEvent> ev;                                    // profiling: before every pass's copies and every decode launch, behind the last
        float copyMs = 0.0f, decodeMs = 0.0f;
    } pcm;
    // clips converted to another rate (zlhip_sound_convert_rate; zl_resample.h): the filter tables on the device, one per (L, M) ever asked for
    struct Resample {
        struct Table { int32_t L = 0, M = 0; ZlDev<float> d; size_t floats = 0; std::vector<float> pending; };   // pending: the host copy, until the call that made the table has waited
        std::vector<Table> tables;
        ZlStageTimer<2> timer; float ms = 0.0f;                     // marks: around the call's launches
    } rs;
    ZlDev<ZlSound> dSounds; ZlDev<ZlClip> dClips;
    ZlDev<ZlVoiceState> dVoices;
    // K1 -> K2 records, double buffered so that planning window i+1 overlaps rendering window i
    struct PlanSet {
        ZlDev<ZlVoiceConst> vconst; ZlDev<ZlRunList> runs; ZlDev<ZlTSeg> tsegs;
        ZlDev<ZlPlanHdr> hdr; ZlDev<ZlPlanSeg0> seg0; ZlDev<ZlPlanSeg1> seg1;
        ZlDev<uint64_t> pairTab;                          // the pair kernels' scalar records of a window (zl_render.h, zl_pair_tab_words), engines in mode 0 only
        ZlDev<double> ctlP; ZlDev<float> ctlEnv;          // the window's pool of per-frame control slots (zl_plan.h, zl_ctl_alloc)
        ZlDev<unsigned long long> ctlNext;                // its bump counter, never reset: a window's slots count from ctlBase
        unsigned long long ctlBase = 0;                   // host side: past every value the counter can have reached
        ZlDev<ZlSimConst> simConst;
        ZlDev<float> partials;
        ZlDev<int32_t> order; size_t orderInts = 0;       // K2's phase order of the window's blocks (K1o): [z-slots][K] and the run summary behind it (zl_order_ints), allocated on first use
        ZlEvent planned, rendered, k1done;
        hipEvent_t renderedEv = nullptr; // alias: the event that marks the end of the last rendering from this set (rendered, or a profiling event)
        bool used = false;               // `rendered` has been recorded at least once
    } ps[2];
    int windowBlocks = 0;                // plan_window_blocks when given (a fixed number of blocks per plan window)
    size_t windowFrames = 0;             // else a window is this many frames: 2048 blocks of 256 frames, more blocks when they are shorter
    int windowCap = 0;                   // blocks the K1 -> K2 record arrays hold
    size_t ctlPoolFrames = 0;            // frames of per-frame control a record set's pool holds (slots = this / nframes)
    int ctlSlotsOverride = -1;           // ZL_CTL_POOL_SLOTS (tests of the exhausted pool)
    ZlStream planStream;                 // K0 + K1 (sequential per voice)
    hipStream_t lastRenderStream = nullptr;                          // alias: the stream the previous call rendered on
    hipStream_t lastPlanStream = nullptr;                            // alias: where the previous call planned (voice-state order)
    ZlEvent evPlanTail;                  // the end of that planning, where it ran on the planning stream
    hipEvent_t lastPlanEvent = nullptr;  // alias: marks the end of that planning: evPlanTail, or the call's `done` event when it planned on its render stream
    ZlStream asmStream;                  // K1c of window w runs here, next to K1 of window w+1
    std::vector<std::pair<int, int>> wins;
    // Per-call resources, double buffered so that consecutive zlhip_render_batch calls pipeline: the host prepares
    // (and the planning stream plans) call i+1 while call i still renders; a slot is reused by call i+2.
    struct CallSlot {
        ZlMapped<ZlClock> clocks;        // the call's block clocks, in host memory mapped into the device: K1 reads them in place
        ZlMapped<ZlPassParams> pass; ZlDev<ZlPassParams> dPass;   // fused fan-out parameters of the call
        // the call's voice operations, in host memory mapped into the device: K0 reads them in place (no copy command)
        ZlMapped<ZlVoiceOp> ops; ZlMapped<ZlOpRange> ranges;
        ZlMapped<ZlClipEdit> edits;      // the call's clip-parameter edits, same arrangement
        ZlMapped<ZlReport> reports; ZlDev<ZlReport> dReports;
        ZlMapped<float> gain;
        ZlMapped<ZlBatchStats> stats; ZlDev<ZlBatchStats> dStats;
        ZlEvent evBegin, evEnd;
        hipEvent_t done = nullptr;       // alias: doneEv[doneGen]
        // `done` alternates between two events from one use of the slot to the next, so that the NEXT call (the other slot) can take this
        // call's completion as the begin of its own profile -- one event-record packet fewer between two calls' render kernels -- and
        // still find it intact when it is harvested, two calls later
        ZlEvent doneEv[2]; unsigned doneGen = 0;
        hipEvent_t beginEv = nullptr;    // alias: what this call's profile counts from: its own evBegin, or the previous call's `done`
        std::vector<ZlEvent> evK2;       // [2 * max windows] start/end of every K2 launch (profiling)
        int windows = 0;
        bool inflight = false, profiled = false;
        bool fusedDone = false;          // the call's last K2 launch published the reports and carries `done` as its stop event (no report kernel)
    } slots[2];
    unsigned callIndex = 0, setPhase = 0;
    CallSlot *latest = nullptr;          // slot of the most recent call
    zlhip_timings totals{}; int totalCalls = 0;   // sums over harvested calls (zlhip_profile_totals)
    ZlDev<float> dGain;
    ZlDev<ZlPassCache> dPassCache;       // per voice: the recorded pass of its loop (zl_plan.h, replay_cached_pass)
    ZlDev<float> dBus;
    ZlDev<ZlBlockLevels> dLevels; ZlDev<ZlLevelsState> dLevelState;
    ZlDev<int32_t> dTrace; ZlDev<ZlPassParams> dPass;
    size_t traceInts = 0;
    int maxGroups = 1;

    // pinned host staging
    ZlMapped<float> hBus;                // one real-time block, host memory mapped into the device
    // one real-time block's JackPassthrough fan-out [B][6][max_frames] (zlhip_render_fanout), written by the kernels like hBus; the
    // parameter table the resident kernel reads ([B], mapped host memory) and its version (never 0; moved when an entry changes)
    ZlMapped<float> hFan;
    ZlMapped<ZlPassParams> hPassRt;
    ZlMapped<uint32_t> hNonFinite;       // mapped host word: zl_k_interleave sets it when an uploaded sample is NaN or infinite
    uint32_t passSeq = 1;
    // zero-copy delivery of a real-time cycle: when the caller's out_left / out_right (/ fan_out) are page-locked and mapped (zlhip_host_alloc,
    // hipHostMalloc, hipHostRegister) the kernels write them directly -- no copy on the host behind the cycle (24 KB + 72 KB for 12 buses:
    // 1.6 + 5 us of reading lines the device has just written).  The device views of the last buffers seen are kept.
    struct OutViews { const void *hL = nullptr, *hR = nullptr, *hF = nullptr; float *dL = nullptr, *dR = nullptr, *dF = nullptr; bool ok = false; } outViews;
    bool directOut = true;               // ZL_RT_DIRECT_OUT=0: always through the staging rows
    ZlMapped<ZlLevelsState> hLevelState;

    // host mirrors
    ZlHostControl hc;                    // voices / sounds / clip parameters / pending ops (zl_host.h)
    std::vector<ZlOpRange> ranges;

    // last batch
    int lastK = 0, lastN = 0, lastWindows = 0; float *lastBus = nullptr; bool outstanding = false; bool reportsFresh = false;
    bool trace = false; int traceK = 0, traceN = 0;
    int forceSlow = 0;
    size_t deviceBytes = 0;              // HBM the engine allocated at creation (arena included), and since then in scratch[], rate-conversion tables and arena segments
    int staged = 0;                      // K2 variant with LDS-staged source windows (zl_kernels.hip), chosen per mode at creation

    // resident real-time kernel (zl_k_rt_loop): the mailbox in mapped host memory, its stream, what it was launched for
    struct Rt {
        bool enabled = false, running = false; int wide = -1;    // wide: 1 always, 0 never, -1 only with one voice per workgroup
        ZlMapped<ZlRtShared> mail;                         // the mailbox; with dev, devRanges and stream made by the first start, all or none (rt_start)
        ZlDev<ZlRtDev> dev;                                // the kernel's own hand-off words in HBM
        ZlDev<ZlOpRange> devRanges;                        // wide buses: workgroup 0's copy of a block's operation ranges
        int capacity[2] = {-1, -1};                        // workgroups of the kernel the device holds at once (narrow, wide); -1 = not asked yet
        int vw = 0;                                        // wide buses: voices per resident workgroup (a divisor of voices_per_bus)
        double share = 0.0;                                // of the device's resident-workgroup capacity this engine's kernel takes (rt_eligible)
        std::atomic<bool> inCycle{false};                  // a cycle is being rendered through the resident kernel (its share stays taken even if the kernel has just left)
        int maxFrames = 4096;                              // longest period the resident kernel takes (ZL_RT_MAX_FRAMES)
        ZlStream stream;
        int nframes = 0;
        unsigned long long seq = 0;
        unsigned long long starts = 0, cycles = 0;        // launches of the resident kernel, cycles it rendered (zlhip_rt_stats)
        unsigned long long idleTicks = 20000000ull;       // 200 ms of the 100 MHz counter without a block: the kernel leaves
        bool stampsOn = false; double stampSum[6] = {0, 0, 0, 0, 0, 0}; unsigned long long stampN = 0;   // ZL_RT_STAMPS=1: stage times (us)
        // where the last real-time cycle spent its time, seen from the host (zlhip_rt_last_cycle): a worst case has to be attributable
        bool traceOn = false; double slowUs = 0.0;         // ZL_RT_TRACE=1; ZL_RT_TRACE_SLOW_US=<n>: cycles longer than that are reported on stderr
        zlhip_rt_cycle_trace last{};
    } rt;

    // offline bounce (zlhip_bounce): the device bus buffers of two chunks rendered into in turn, their 16-bit versions, the copy stream.
    // A chunk is ONE zlhip_render_batch call; every plan window of it is delivered as soon as its render kernel has finished
    // (the sink below, called from the window loop), while the following windows render.
    struct Bounce {
        static constexpr int NBUF = 2, NEV = 16;
        ZlDev<float> bus[NBUF]; ZlDev<int16_t> pcm[NBUF];
        size_t busFloats = 0, pcmFrames = 0;               // what every buffer that exists holds
        ZlStream copyStream;
        ZlEvent copied[NBUF];                              // the last delivery out of a chunk buffer
        ZlEvent winEv[NEV];                                // "window rendered (and converted)": waited for by the copy stream
        unsigned winNext = 0;
        bool active = false;                 // inside zlhip_bounce: every chunk plans on the planning stream
        struct Sink {
            bool on = false, pcm = false;
            char *hostBase = nullptr;        // the chunk's first frame in the caller's buffer
            void *hostDev = nullptr;         // direct delivery: the device view of hostBase (page-locked memory only), else nullptr
            size_t totalFrames = 0;          // frames per row of the caller's buffer (the whole bounce)
            int16_t *pcmDev = nullptr;       // the chunk's 16-bit staging buffer [B][chunk frames][2]
        } sink;
    } bnc;

    bool failed = false;                 // the resident kernel stopped answering in the middle of a cycle: the voice table is undefined (zlhip_render)

    // profiling
    bool profiling = false; ZlEvent evJoin;
    hipEvent_t joins[2] = {nullptr, nullptr};   // alias: events on caller streams the host still has to wait for (engine_wait)
    zlhip_timings timings{};
};

#define ZL_HIP(e, call)                                                                        \
    do {                                                                                       \
        hipError_t st_ = (call);                                                               \
        if (st_ != hipSuccess) {                                                               \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(st_);                     \
            return ZLHIP_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

#define ZL_KERNEL(e, call)                                                                     \
    do {                                                                                       \
        int st_ = (call);                                                                      \
        if (st_ != 0) {                                                                        \
            (e)->err = std::string(#call) + ": " + hipGetErrorString((hipError_t)st_);         \
            return ZLHIP_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

#pragma GCC visibility push(hidden)
// hipFree, hipHostFree and hipDeviceSynchronize wait for every resident kernel on the device: while one of these lives, the other
// engines' kernels have stepped aside (zl_engine.cpp, "resident kernels and device-synchronising HIP calls")
struct ZlQuiesce {
    explicit ZlQuiesce(const zlhip_engine *self);
    ~ZlQuiesce();
    ZlQuiesce(const ZlQuiesce &) = delete;
    ZlQuiesce &operator=(const ZlQuiesce &) = delete;
};

int fail(zlhip_engine *e, int code, const char *msg);
int engine_wait(zlhip_engine *e);
int rt_stop(zlhip_engine *e);
int call_begin(zlhip_engine *e, bool stop);
int grow_buf(zlhip_engine *e, GrowBuf &b, size_t need, size_t elem, size_t new_cap, bool twin, const char *what);
int alloc_extent(zlhip_engine *e, size_t floats, size_t *out_off);
void free_extent(zlhip_engine *e, size_t off, size_t n);
float *arena_ptr(const zlhip_engine *e, uint64_t off);
void adopt_sound(zlhip_engine *e, int id, const ZlSound &s, size_t floats);
#pragma GCC visibility pop
