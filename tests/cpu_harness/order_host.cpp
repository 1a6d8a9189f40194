// Host build of K2's phase order (libzl_amd/csrc/zl_order.h) for the CPU tier -- TEST HARNESS ONLY.
// zlord_build replays K1o (zl_kernels.hip) per z-slot: the key voice, its buckets, the counting sort.
#include <climits>
#include <cstring>
#include <vector>

#include "zl_host.h"
#include "zl_order.h"

extern "C" {

// runs of V voices given as arrays; order and bucket are [nslots][K] (bucket: the key voice's bucket of order[z][j], -1 in a slot kept
// in time order); key_voice[z]: the slot's key voice or -1.  Returns the number of sorted slots.
int zlord_build(int V, int VPB, int NB, int nslots, int K, int N, const int *per_t0, const int *per_M, const int *per_n,
                const int *dead_from, int *order, int *bucket, int *key_voice)
{
    std::vector<ZlRunList> runs((size_t)V);
    for (int v = 0; v < V; ++v) {
        std::memset(&runs[(size_t)v], 0, sizeof(ZlRunList));
        runs[(size_t)v].per_t0 = per_t0[v]; runs[(size_t)v].per_M = per_M[v]; runs[(size_t)v].per_n = per_n[v];
        runs[(size_t)v].dead_from = dead_from[v];
    }
    std::vector<int> hist(ZL_ORDER_MAXBKT);
    int sorted = 0;
    for (int z = 0; z < nslots; ++z) {
        int vb, ve;
        zl_order_slot_voices(z, NB, VPB, V, vb, ve);
        int kv = -1;
        for (int v = vb; v < ve && kv < 0; ++v) if (zl_order_is_key(runs[(size_t)v], K)) kv = v;
        ZlOrderKey key;
        const bool on = kv >= 0 && zl_order_setup(runs[(size_t)kv], K, N, key);
        key_voice[z] = kv;
        int *o = order + (size_t)z * K;
        zl_order_sort_host(on ? &key : nullptr, K, hist.data(), o);
        for (int j = 0; j < K; ++j) bucket[(size_t)z * K + j] = on ? zl_order_bucket(key, o[j]) : -1;
        sorted += on ? 1 : 0;
    }
    return sorted;
}

int zlord_shape(int groups, int staged, int nblocks, int nframes) { return zl_order_shape(groups, staged, nblocks, nframes) ? 1 : 0; }

int zlord_window(int mode, int shape, int bounce, int nframes, int K, double loop_frames)
{
    return zl_order_window(mode, shape != 0, bounce != 0, nframes, K, loop_frames) ? 1 : 0;
}

// ZlHostControl::phase_order_loop_frames over voices described by arrays (voice v plays clip v)
double zlord_loop_frames(int V, double fs, const int *playing, const int *cheap, const int *looping, const float *length_seconds)
{
    ZlHostControl hc;
    hc.init(1, V, V, fs);
    for (int v = 0; v < V; ++v) {
        hc.clipParams[(size_t)v].length_seconds = length_seconds[v];
        ZlHostVoice &hv = hc.voices[(size_t)v];
        hv.isPlaying = playing[v] != 0; hv.cheapPlan = cheap[v] != 0; hv.cmd.looping = looping[v]; hv.sound = v; hv.hasCommand = true;
    }
    return hc.phase_order_loop_frames();
}

}
