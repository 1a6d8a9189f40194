"""What the loop finder's device tests share (tests/test_loop_gpu.py, tests/test_loop_edges_gpu.py): a call's costs, item records and
results against the numpy / Python-integer restatement (tests/loop_ref.py) -- every integer bit for bit, the three dB fields within
1e-9."""
import numpy as np

import loop_ref as lr

SR = 48000.0


def upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def played(syn, cid):
    """the clip's playback data as the engine holds it, planar"""
    L, R = syn.read_clip(cid)
    return np.stack([L, R]) if R is not None else L[None, :]


def want(src, rate, r):
    return lr.loop(src, rate, *(r.get(k, 0) for k in lr.KEYS), want=True)


def same(got, res):
    return all(int(got[k]) == int(res[k]) for k in lr.RESULT_INTS) and all(abs(float(got[k]) - float(res[k])) <= 1e-9 for k in lr.RESULT_DBS)


def check_batch(syn, reqs, srcs, costs=True, rates=None, cache=None):
    """reqs: dicts with "clip" and zlhip_loop_request's fields; srcs: {clip: planar}; rates: {clip: rate} where it is not SR.  The costs,
    the item records and the result of every request against the restatement (kept in `cache`, a dict, per request where one is given:
    a restatement is computed once); returns the mismatches and the results"""
    bad = []
    outs = syn.clip_loop_batch(reqs)
    for i, (r, got) in enumerate(zip(reqs, outs)):
        key = tuple(sorted(r.items()))
        if cache is None or key not in cache:
            w = want(srcs[r["clip"]], (rates or {}).get(r["clip"], SR), r)
            if cache is not None:
                cache[key] = w
        else:
            w = cache[key]
        res, items, cost = w
        okI = syn.loop_items(i) == items
        okC = True
        if costs:
            c = syn.loop_costs(i)
            okC = c.dtype == np.uint32 and c.shape == cost.shape and np.array_equal(c.astype(np.int64), cost)
        if not (okI and okC and same(got, res)):
            bad.append((srcs[r["clip"]].shape, r, "items" if not okI else "costs" if not okC else ("result", got, res)))
    return bad, outs
