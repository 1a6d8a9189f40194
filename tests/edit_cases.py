"""The clip edit's cases, shared by the CPU tier (tests/test_edit_cpu.py walks them through the host build of the header) and the GPU
tier (tests/test_edit_gpu.py runs them through the kernels): each a dict with the planar clip "x", the request's fields "q"
(edit_ref.request) and a "tag" that says which edge it is aimed at."""
import numpy as np

import edit_ref as er

f32 = np.float32
SR = 48000.0
THR = float(er.THRESHOLD)


def clip(rng, ch, n):
    x = rng.uniform(-1.0, 1.0, (ch, n)).astype(f32)
    special = np.array([0.0, -0.0, 1e-39, -1e-39, 1.0, -1.0], f32)
    at = rng.integers(0, n, size=max(1, n // 7))
    x[rng.integers(0, ch, size=at.size), at] = special[rng.integers(0, special.size, size=at.size)]
    return x


def quiet(rng, ch, n, thr=THR):
    """noise below the threshold, nowhere zero: a float that leaks shows"""
    return (rng.uniform(0.1, 0.5, (ch, n)) * rng.choice([-1.0, 1.0], (ch, n)) * thr).astype(f32)


def grid(seed=1):
    """Copy, reverse and fades: mono and stereo, forward and reversed, with a' channels and n channels in every residue modulo 4 and the
    clip ending at b' or 5 frames behind it; n = 1 .. 5; a' = 0 reversed; the whole clip reversed; fades of 0, 1 and 2 frames; both fades
    asked far too long on n = 9 and n = 10 under all three curves; a mono clip of 3000 frames (3 render workgroups) and a reversed stereo
    one of 2000 (4) whose fades cross a workgroup's edge.  Trim: see the tags.  Identity and silent requests first, last and twice in a
    row."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(tag, x, **q):
        cases.append(dict(tag=tag, x=x, q=er.request(**q)))

    fades = ((0, 0), (1, 0), (0, 2), (2, 1), (1, 2))
    for ch in (1, 2):
        for rev in (0, er.REVERSE):
            for ra in range(4):
                for rn in range(4):
                    a, n = 8 + ra, 40 + rn
                    fi, fo = fades[len(cases) % 5]
                    add("copy", clip(rng, ch, a + n + (0 if (ra + rn) % 2 == 0 else 5)), first_frame=a, num_frames=n, flags=rev, fade_in_frames=fi, fade_out_frames=fo, curve=len(cases) % 3)
            for n in (1, 2, 3, 4, 5):
                add("short", clip(rng, ch, 3 + n + n % 2), first_frame=3, num_frames=n, flags=rev, fade_in_frames=1, fade_out_frames=1, curve=n % 3)
            for n in (9, 10):
                for curve in (er.LINEAR, er.SQRT, er.SMOOTH):
                    add("long fades", clip(rng, ch, n + 4), first_frame=2, num_frames=n, flags=rev, fade_in_frames=1000, fade_out_frames=1000000, curve=curve)
        add("from 0 reversed", clip(rng, ch, 50), first_frame=0, num_frames=37, flags=er.REVERSE)
        add("whole reversed", clip(rng, ch, 61), flags=er.REVERSE)
    add("workgroup edge", clip(rng, 1, 3100), first_frame=7, num_frames=3000, fade_in_frames=1100, fade_out_frames=1000, curve=er.SMOOTH)
    add("workgroup edge", clip(rng, 2, 2050), first_frame=33, num_frames=2000, flags=er.REVERSE, fade_in_frames=600, fade_out_frames=520, curve=er.SQRT)

    def trim(tag, ch, n, a, num, put, thr=0.0, flags=er.TRIM, **q):
        """a quiet clip with the samples of `put` {(channel, frame): value}"""
        x = quiet(rng, ch, n, THR if thr == 0.0 else thr)
        for (c, f), v in put.items():
            x[c, f] = v
        add(tag, x, first_frame=a, num_frames=num, flags=flags, threshold=thr, **q)

    for ch in (1, 2):
        c1 = ch - 1
        trim("loud at the first frame", ch, 300, 11, 200, {(0, 11): 0.5, (c1, 100): 0.25})
        trim("loud at the last frame", ch, 300, 11, 200, {(c1, 60): 0.5, (0, 210): 0.25})
        trim("at the threshold", ch, 200, 5, 150, {(c1, 70): f32(0.01)}, thr=0.01)
        trim("below the threshold", ch, 200, 5, 150, {(c1, 40): np.nextafter(f32(0.01), f32(0.0)), (0, 90): 0.5}, thr=0.01)
        trim("negative", ch, 200, 5, 150, {(c1, 33): -0.3, (0, 120): -THR})
        for v in (np.nan, np.inf, -np.inf):
            trim("non-finite", ch, 120, 3, 100, {(c1, 50): v})
        # the frames in front of and behind the region are loud and share their 16-byte groups with it
        trim("loud neighbours", ch, 300, 13, 201, {(0, 12): 0.9, (c1, 12): -0.9, (0, 214): 0.9, (c1, 214): 0.9, (0, 50): 0.5, (c1, 180): 0.5})
        trim("loud neighbours of a silent region", ch, 300, 13, 201, {(0, 12): 0.9, (c1, 12): np.inf, (0, 214): 0.9, (c1, 214): np.nan})
        trim("no room", ch, 400, 20, 300, {(0, 100): 0.5, (c1, 200): 0.5}, pre_roll_frames=10000, hold_frames=2 ** 31 - 1)
        trim("pre-roll and hold", ch, 400, 20, 300, {(0, 100): 0.5, (c1, 200): 0.5}, pre_roll_frames=7, hold_frames=13, flags=er.TRIM | er.REVERSE, fade_in_frames=5, fade_out_frames=9)
        a = 5
        trim("chunk edge, last frame", ch, 4300, a, 4200, {(c1, a + er.CHUNK - 1): 0.5})
        trim("chunk edge, first frame", ch, 4300, a, 4200, {(c1, a + er.CHUNK): 0.5})
        trim("chunk edge, both", ch, 4300, a, 4200, {(0, a + er.CHUNK - 1): 0.5, (c1, a + er.CHUNK): 0.5})
        trim("silent middle chunk", ch, 3 * er.CHUNK + 100, 3, 3 * er.CHUNK + 50, {(0, 1000): 0.5, (c1, 2 * er.CHUNK + 900): 0.5}, pre_roll_frames=3, hold_frames=2)
    trim("right channel only", 2, 300, 10, 250, {(1, 77): 0.5, (1, 140): -0.5})

    def silent():
        x = quiet(rng, 1 + len(cases) % 2, 300)
        return dict(tag="silent", x=x, q=er.request(first_frame=len(cases) % 7, num_frames=250, flags=er.TRIM | er.REVERSE, fade_in_frames=4))

    def identity(trimmed):
        x = clip(rng, 1 + len(cases) % 2, 200)
        x[:, 0] = 0.5
        x[:, -1] = 0.5
        return dict(tag="identity", x=x, q=er.request(flags=er.TRIM if trimmed else 0, pre_roll_frames=3))

    half = len(cases) // 2
    return [identity(False)] + cases[:half] + [silent(), identity(True)] + cases[half:] + [silent()]


def want(c, w_in=None, w_out=None):
    """the restatement of one case: (result, the extent's floats)"""
    res, y = er.edit(c["x"], c["q"], w_in, w_out)
    return res, er.extent(y)


def facts(cases):
    """what the grid is meant to cover, counted from the restatement's results"""
    F = dict(copy=set(), short=set(), fades=set(), curves=set(), tags=set(), from0rev=0, at_end=0, whole_rev=0, odd_middle=0, even_all=0,
             wg_edge=0, wgs=0, silent=0, identity=0, scan_chunks=0, first_is_F=0, last_is_Z=0)
    for c in cases:
        ch, length = c["x"].shape
        q = c["q"]
        res, _ = er.edit(c["x"], q)
        F["tags"].add(c["tag"])
        F["silent"] += res["silent"]
        F["identity"] += (not res["applied"]) and (not res["silent"])
        if q["flags"] & er.TRIM:
            a, b, _ = er.resolve(length, q)
            F["scan_chunks"] = max(F["scan_chunks"], -(-(b - a) // er.CHUNK))
            F["first_is_F"] += res["first_loud"] == a
            F["last_is_Z"] += res["last_loud"] == b - 1
        if not res["applied"]:
            continue
        a2, n, rev = res["first_frame"], res["num_frames"], res["reversed"]
        Xi, Xo = res["fade_in_frames"], res["fade_out_frames"]
        F["copy"].add((ch, rev, a2 * ch % 4, n * ch % 4))
        F["short"].add((ch, rev, n) if n <= 5 else None)
        F["fades"].update((Xi, Xo) if max(Xi, Xo) <= 2 else ())
        F["curves"].add(q["curve"] if Xi or Xo else None)
        F["from0rev"] += bool(rev and a2 == 0 and n < length)
        F["at_end"] += a2 + n == length
        F["whole_rev"] += bool(rev and a2 == 0 and n == length)
        F["odd_middle"] += n % 2 == 1 and Xi == Xo == n // 2 and q["fade_in_frames"] > n
        F["even_all"] += n % 2 == 0 and Xi == Xo == n // 2 and q["fade_in_frames"] > n
        groups = (((n + er.PAD) * ch + 3) // 4)
        F["wgs"] = max(F["wgs"], -(-groups // er.WG))
        per = 4 * er.WG // ch
        F["wg_edge"] += (Xi > per) + (Xo > 0 and (n - Xo) // per < (n - 1) // per and (n - Xo) % per != 0)
    return F


# ---- on the device --------------------------------------------------------------------------------------------------------------------
def upload(syn, x, sr=SR):
    return syn.register_clip(x[0].copy(), x[1].copy() if x.shape[0] == 2 else None, float(sr))


def dirty(syn, floats):
    """noise over the first `floats` floats of a fresh arena, released again: what is allocated next lies on it, so that a float of an
    extent that nobody writes does not read as zero by luck"""
    x = np.random.default_rng(99).uniform(1.0, 2.0, floats - 8).astype(f32)
    cid = syn.register_clip(x, None, SR)
    syn.unregister_clip(cid)


def same_bits(got, ext):
    """None, or where two extents differ (NaN payloads differ between the host and the device: a NaN equals a NaN)"""
    u32 = np.uint32
    if got.size != ext.size:
        return ("extent size", got.size, ext.size)
    an, bn = np.isnan(got), np.isnan(ext)
    if not np.array_equal(an, bn) or not np.array_equal(got[~an].view(u32), ext[~bn].view(u32)):
        return ("extent", np.flatnonzero((got.view(u32) != ext.view(u32)) & ~(an & bn))[:8])
    return None


def mismatch(syn, cid, c, got):
    """what differs between the device's answer for case c (result `got`, the extent clip `cid` holds now) and the restatement, or None"""
    res, ext = want(c)
    if any(got[k] != res[k] for k in er.RESULT_FIELDS):
        return ("result", got, res)
    now = syn.clip_extent(cid)
    if not res["applied"]:                                         # (its upload's extent: the floats behind the zero frames are not the edit's to write)
        return same_bits(now[:c["x"].size], ext[:c["x"].size]) if now.size == ext.size else ("extent size", now.size, ext.size)
    return same_bits(now, ext)


def check_call(syn, cases, ids):
    """one clip_edit_batch over the cases (clip ids[i] holds cases[i]["x"]): (the mismatches, the results)"""
    outs = syn.clip_edit_batch([dict(clip=cid, **c["q"]) for cid, c in zip(ids, cases)])
    bad = []
    for i, (cid, c, got) in enumerate(zip(ids, cases, outs)):
        m = mismatch(syn, cid, c, got)
        if m is not None:
            bad.append((i, c["tag"], c["x"].shape, c["q"], m))
    return bad, outs
