"""Calls of the overview, onset and decode services that are large enough for a wavefront to take a RUN of items, shared by the CPU tier
(tests/test_capped_runs_cpu.py asserts every case's predicates and its item counts from the host builds of the headers) and the GPU tier
(tests/test_capped_runs_gpu.py runs the cases through the kernels).  DESIGN.md section 9 ("The run") says what a run is.

zl_k_overview_reduce, zl_k_onset_energy and zl_k_pcm_decode each stop growing their grid at ZL_*_MAX_BLOCKS workgroups; above that wave w
of nwaves takes the items [it, end):

    q = items // nwaves, rem = items - q nwaves, it = w q + min(w, rem), end = it + q + (w < rem)

finds the record (request, piece) of `it` by bisection over the records' bases and steps to the next record inside the run.  The host
walks of tests/cpu_harness visit items one by one and never form a run, so only calls of more than nwaves items, run on the device, see
this code.  partition() restates the formula; nwaves is read from the three .hip files as text, so a changed cap fails the predicates
of the CPU tier instead of silently leaving the regime.

A case is a dict: service, total, specs (one tuple per record), items and bases (int64 per record), and what the service needs besides.
Cases are many records over a few small sources; records overlap and repeat a source, which keeps the data at a few MB.

The totals.  16384 waves: 16384 and 16385 items give q = 1 with rem = 0 and 1, 32767 gives q = 1 with rem = nwaves - 1, 32768 and 32769
give q = 2 with rem = 0 and 1, 3 * 16384 + 5 gives q = 3 with a small rem.  A run of these holds at most four items, so it touches at
most four records, and with q = 1, rem = 0 a run is one item and crosses nothing: what CAN be asked of these totals is that a longest run
advances to the next record at every step (max_records == longest).  8 * 16384 + 3 (q = 8, rem = 3) is here for the runs of eight and
nine items: a run that touches eight records and more, the overview's whole pass narrow -> one piece per column -> several pieces ->
narrow inside one run, and decode's verdict pieces of two items each inside one run.

No total is left out for a limit: the largest call is 131075 hops (limit 4194304 per call, 65536 per request), below 262144 columns
(4096 per request), and its PCM fits the default stage in one pass; limits() asserts that per case.
"""
import functools
import os
import re

import numpy as np

import decode_ref as dr
import onset_ref as onr
import overview_ref as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libzl_amd", "csrc")
f32, u32 = np.float32, np.uint32

SERVICES = {"overview": ("OV", "zl_overview"), "onset": ("ON", "zl_onset"), "decode": ("DEC", "zl_decode")}
# total -> (q, rem) at 16384 waves, written out: a changed cap must fail the comparison, not move the table
TOTALS = {16384: (1, 0), 16385: (1, 1), 32767: (1, 16383), 32768: (2, 0), 32769: (2, 1), 3 * 16384 + 5: (3, 5), 8 * 16384 + 3: (8, 3)}
FIRSTS = (0, 1, 2, 3, 5)


# ---- the launch shape, read from the sources as text ---------------------------------------------------------------------------------
def _define(text, name):
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+\(?[ \t]*(\d+)[ \t]*u?[ \t]*(?:<<[ \t]*(\d+))?[ \t]*\)?[ \t]*(?://.*)?$" % re.escape(name), text, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0][0]) << int(found[0][1] or 0)


@functools.lru_cache(maxsize=None)
def launch_shape(service):
    """{MAX_BLOCKS, THREADS, WAVE} of the service's run kernel"""
    tag, stem = SERVICES[service]
    text = "\n".join(open(os.path.join(CSRC, stem + ext)).read() for ext in (".hip", ".h"))
    return {k: _define(text, "ZL_%s_%s" % (tag, k)) for k in ("MAX_BLOCKS", "THREADS", "WAVE")}


@functools.lru_cache(maxsize=None)
def header_value(service, name):
    tag, stem = SERVICES[service]
    return _define(open(os.path.join(CSRC, stem + ".h")).read(), "ZL_%s_%s" % (tag, name))


def grid_waves(service, items):
    """waves of the launch: one per item, four to a workgroup, until the grid stops growing"""
    s = launch_shape(service)
    per = s["THREADS"] // s["WAVE"]
    return min(-(-items // per), s["MAX_BLOCKS"]) * per


def partition(items, nwaves):
    """every wave's run [it, end) as two int64 arrays"""
    w = np.arange(nwaves, dtype=np.int64)
    q = items // nwaves
    rem = items - q * nwaves
    it = w * q + np.minimum(w, rem)
    return it, it + q + (w < rem)


def facts(bases, total, nwaves):
    """what the runs of a call do to its records"""
    bases = np.asarray(bases, np.int64)
    it, end = partition(total, nwaves)
    live = end > it
    it, end = it[live], end[live]
    r0 = np.searchsorted(bases, it, "right") - 1                   # the bisection: the last record whose base is <= it
    r1 = np.searchsorted(bases, end - 1, "right") - 1
    on = bases[r0] == it
    q = total // nwaves
    return dict(q=int(q), rem=int(total - q * nwaves), longest=int((end - it).max()), crossing=int((r1 > r0).sum()),
                max_records=int((r1 - r0 + 1).max()), on_base=bool(on.any()), off_base=bool((~on).any()),
                mid_to_later=bool((~on & (r1 > r0)).any()), mid_through=bool((~on & (r1 - r0 >= 2)).any()),
                full_advance=bool(((r1 - r0 + 1 == end - it) & (end - it == (end - it).max())).any()))


def run_of(total, nwaves, item):
    """the wave whose run holds the item"""
    it, end = partition(total, nwaves)
    w = int(np.searchsorted(it, item, "right") - 1)
    while end[w] <= item:                                          # (empty runs share their start with the next one)
        w += 1
    return w


def runs_classes(bases, classes, total, nwaves):
    """per run that crosses a record boundary: the classes of its records, in order, without repeats"""
    bases = np.asarray(bases, np.int64)
    it, end = partition(total, nwaves)
    r0 = np.searchsorted(bases, it, "right") - 1
    r1 = np.searchsorted(bases, np.maximum(end, it + 1) - 1, "right") - 1
    out = []
    for w in np.flatnonzero((end > it) & (r1 > r0)):
        seq = [classes[r0[w]]]
        for r in range(r0[w] + 1, r1[w] + 1):
            if classes[r] != seq[-1]:
                seq.append(classes[r])
        out.append(tuple(seq))
    return out


# ---- assembling a call ---------------------------------------------------------------------------------------------------------------
# a motif: stretches of one-item records between records of a few and of many items
SHAPE = (("one", 12), ("many", 37), ("one", 9), ("many", 2), ("many", 3), ("one", 8), ("many", 100), ("many", 5), ("one", 11), ("many", 64), ("one", 10))
WEIGHTS = (3, 1, 4, 1, 5, 9, 2, 6)                                 # the fill between the motifs: uneven, so the motifs meet the runs at changing offsets


def assemble(total, head, one, many, extra, chunk):
    """[(spec, items)]: head, then eight times a motif and its fill, then one one-item record.  one(k) gives the k-th one-item spec,
    many(n, k) a spec of exactly n items; extra: further records of every motif; the fill is cut into records of `chunk` items, and the
    last of them is sized so that the call holds `total` items."""
    recs = list(head)
    k = [0]

    def take(kind, n):
        if kind == "one":
            for _ in range(n):
                recs.append((one(k[0]), 1))
                k[0] += 1
        else:
            recs.append((many(n, k[0]), n))
            k[0] += 1

    fixed = sum(n for _, n in head) + len(WEIGHTS) * (sum(n for _, n in SHAPE) + sum(n for _, n in extra)) + 1
    room = total - fixed
    assert room >= len(WEIGHTS), (total, fixed)
    parts = [room * w // sum(WEIGHTS) for w in WEIGHTS]
    parts[-1] += room - sum(parts)
    for p in parts:
        for kind, n in SHAPE:
            take(kind, n)
        recs.extend(extra)
        while p > 0:
            n = min(p, chunk)
            take("many", n)
            p -= n
    take("one", 1)
    assert sum(n for _, n in recs) == total
    return recs


def _case(service, total, recs, **more):
    items = np.array([n for _, n in recs], np.int64)
    assert (items >= 1).all() and items[0] == 1 and items[-1] == 1
    bases = np.concatenate([[0], np.cumsum(items)[:-1]]).astype(np.int64)
    return dict(service=service, total=total, specs=[s for s, _ in recs], items=items, bases=bases, nwaves=grid_waves(service, total), **more)


def case_facts(c):
    return facts(c["bases"], c["total"], c["nwaves"])


# ---- onset (and tempo, which shares the energy launch) ---------------------------------------------------------------------------
# spec: (clip, first_frame, num_frames, hop); every request runs with ON_REST = (gate, threshold, min_gap, max_onsets)
ON_HOPS = (64, 80, 256, 4096)
ON_REST = (8, 128, 4, 1)
ON_LENGTHS = ((1, 340000), (2, 270000), (1, 9001), (2, 9003))
ON_CHUNK = 4096


def _bursty(ch, length, seed):
    """quiet noise with a burst every few thousand frames: transients to find, no silence"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.01, 0.01, (ch, length))
    for at in range(1500 + 37 * seed, length, 5000 + 611 * seed):
        n = min(1200, length - at)
        x[:, at:at + n] += rng.uniform(-0.45, 0.45, (ch, n)) * np.exp(-np.arange(n) / 300.0)
    return x.astype(f32)


@functools.lru_cache(maxsize=None)
def onset_sources():
    return [_bursty(ch, n, 3 + i) for i, (ch, n) in enumerate(ON_LENGTHS)]


@functools.lru_cache(maxsize=None)
def onset_poison():
    """+-7.9 in every frame: E[h] = hop * 32358^2 (onset_poison_energy), which no hop of a case reaches"""
    return np.random.default_rng(99).choice([-7.9, 7.9], (1, ON_CHUNK * 64 + 8)).astype(f32)


def onset_poison_energy(hop=64):
    return hop * int(onr.quantise(f32(7.9))) ** 2


def onset_poison_requests(clip, hops):
    return [(clip, 0, ON_CHUNK * 64, 64) + ON_REST] * -(-hops // ON_CHUNK)


def on_hops(n, hop):
    return -(-n // hop)


def _on_one(k):
    clip, hop = k % 4, ON_HOPS[(k + k // 4) % 4]
    n = (hop, hop - 1, 1, hop // 2 + 1)[(k // 2) % 4]
    return clip, FIRSTS[k % 5], n, hop


def _on_many(items, k):
    # (clip, hop) pairs in turn; the first that holds the request
    for j in range(8):
        clip, hop = ((0, 64), (1, 64), (0, 80), (1, 256), (2, 64), (3, 80), (0, 4096), (1, 80))[(k + j) % 8]
        first = FIRSTS[k % 5]
        n = items * hop - (0, 1, hop - 1, 7)[k % 4]
        if first + n <= ON_LENGTHS[clip][1]:
            return clip, first, n, hop
    raise AssertionError(items)


@functools.lru_cache(maxsize=None)
def onset_case(total):
    recs = assemble(total, [], _on_one, _on_many, [], ON_CHUNK)
    for (clip, first, n, hop), items in recs:
        assert on_hops(n, hop) == items and first + n <= ON_LENGTHS[clip][1]
    return _case("onset", total, recs)


def onset_requests(c, ids):
    return [(ids[clip], first, n, hop) + ON_REST for clip, first, n, hop in c["specs"]]


@functools.lru_cache(maxsize=None)
def onset_want(spec):
    """the restatement of one request: (onsets, E, N)"""
    clip, first, n, hop = spec
    gate, threshold, min_gap, max_onsets = ON_REST
    return onr.onsets(onset_sources()[clip], first, n, hop, gate, threshold, min_gap, max_onsets)


# ---- overview ------------------------------------------------------------------------------------------------------------------------
# spec: (clip, columns, first_frame, num_frames).  The clips' values lie in disjoint ranges: a column computed from another request's
# record lands outside its own clip's range.
OV_CLIPS = ((1, 170000, (0.25, 0.5)), (2, 170000, (-0.5, -0.25)), (1, 72000, (0.6, 0.9)), (2, 72000, (-0.9, -0.6)))
OV_CHUNK = 4096
# (num_frames, columns, first_frame) that tests/test_overview_cpu.py cuts into several pieces per column
OV_PIECES = ((70001, 1, 0), (70001, 7, 3), (20011, 3, 1), (9973, 2, 5), (4099, 3, 2))


@functools.lru_cache(maxsize=None)
def overview_sources():
    return [np.random.default_rng(40 + i).uniform(lo, hi, (ch, n)).astype(f32) for i, (ch, n, (lo, hi)) in enumerate(OV_CLIPS)]


def ov_ppc(n, columns):
    w = 1 if n <= columns else -(-n // columns)
    return 0 if w <= header_value("overview", "NARROW_FRAMES") else -(-w // header_value("overview", "PIECE_FRAMES"))


def ov_items(n, columns):
    ppc = ov_ppc(n, columns)
    return -(-columns // 64) if ppc == 0 else columns * ppc


def ov_form(n, columns):
    """0: narrow, one lane per column; 1: wide, the piece is the column; 2: wide, several pieces per column"""
    return min(2, ov_ppc(n, columns))


def _ov_one(k):
    columns, n = ((64, 3), (1, 33), (37, 740), (1, 512), (1, 32), (1, 100))[k % 6]      # narrow and one-piece columns in turn
    return k % 4, columns, FIRSTS[k % 5], n


def _ov_many(items, k):
    first = FIRSTS[k % 5]
    if k % 3 == 0 and items <= 64:
        columns = 64 * items - (0, 1, 13)[(k // 3) % 3]
        return k % 4, columns, first, (3 if k % 2 else 2 * columns)
    if k % 3 == 2 and items % 2 == 0 and items // 2 * 700 + first <= 72000:
        return k % 4, items // 2, first, items // 2 * 700
    clip = k % 4 if items * 512 + first <= 72000 else k % 2
    for w in ((33, 40, 100, 512) * 2)[k % 4:]:
        if items * w + first <= OV_CLIPS[clip][1]:
            return clip, items, first, items * w
    return clip, items, first, items * 33


def _ov_extra():
    """every motif also holds: narrow, one piece, two pieces in turn at both parities; 4096 columns over three frames; the piece geometry"""
    forms = lambda i: [((i % 4, 64, FIRSTS[i % 5], 3), 1), (((i + 1) % 4, 1, FIRSTS[(i + 2) % 5], 100), 1), (((i + 2) % 4, 1, FIRSTS[(i + 1) % 5], 777), 2)]
    out = []
    for i in range(6):
        out += forms(i)
    out.append(((3, 64, 1, 3), 1))
    for i in range(6):
        f = forms(i + 1)
        out += [f[1], f[2], f[0]]
    out.append(((0, 4096, 1, 3), 64))
    for i, (n, columns, first) in enumerate(OV_PIECES):
        out.append(((2 + i % 2, columns, first, n), ov_items(n, columns)))
    return out


@functools.lru_cache(maxsize=None)
def overview_case(total):
    recs = assemble(total, [], _ov_one, _ov_many, _ov_extra(), OV_CHUNK)
    for (clip, columns, first, n), items in recs:
        assert ov_items(n, columns) == items and first + n <= OV_CLIPS[clip][1], (clip, columns, first, n, items)
    return _case("overview", total, recs, forms=[ov_form(n, columns) for (_, columns, _, n), _ in recs])


def overview_requests(c, ids):
    return [(ids[clip], columns, first, n) for clip, columns, first, n in c["specs"]]


@functools.lru_cache(maxsize=None)
def overview_want(spec):
    clip, columns, first, n = spec
    return ov.overview(overview_sources()[clip], columns, first, n)


def overview_facts(c):
    seqs = runs_classes(c["bases"], c["forms"], c["total"], c["nwaves"])
    steps = {(a, b) for s in seqs for a, b in zip(s, s[1:])}

    def holds(s, pattern):
        return any(s[i:i + len(pattern)] == pattern for i in range(len(s)))
    return dict(forms_in_one_run=max([len(set(s)) for s in seqs], default=1), steps=steps, whole_pass=any(holds(s, (0, 1, 2, 0)) for s in seqs))


# ---- decode --------------------------------------------------------------------------------------------------------------------------
# spec: (format, channels, length, source) -- source "pool": the first `length` frames of the pool of (format, channels); otherwise one
# of the verdict pieces.  A clip is one piece (the call is one pass), so a record is a clip.
DEC_CHUNK = 2048
DEC_SMALL = ((dr.U8, 1), (dr.S16, 2), (dr.U8, 2), (dr.S16, 1))    # the fill: one or two bytes per sample, so the largest call fits the stage
DEC_VERDICT = ("f32_inf", "s16", "f32_clean", "f64_1e300")         # in this order inside one run
PLACEMENTS = ("last", "first")                                     # the non-finite sample lies in the last / the first item of its piece


def dec_items(ch, length):
    oc = min(2, ch)
    return -(-((((length + dr.PAD) * oc + 3) & ~3) // 4) // 64)


def _dec_length(items, oc, short):
    """frames of a clip of `items` items whose last item holds 64 - short / 4 groups (short: floats, a multiple of 4 below 256)"""
    return (256 * items - short) // oc - dr.PAD


def _dec_one(k):
    ch = 3 if k % 7 == 6 else 1 + k % 2
    length = ((248, 100, 1, 247, 5) if ch == 1 else (120, 50, 3, 119, 2))[k % 5]        # 248 mono / 120 stereo frames: exactly 64 groups
    return dr.FORMATS[k % 6], ch, length, "pool"


def _dec_many(items, k):
    fmt, ch = DEC_SMALL[k % 4] if items > 256 else (dr.FORMATS[k % 6], 1 + k % 2)
    return fmt, ch, _dec_length(items, ch, ((0, 100, 252) if items > 1 else (0, 100, 200))[k % 3]), "pool"


def _dec_head(total, nwaves):
    """the four verdict pieces at the start of a longest run: wave 0's while a run is shorter than six items (pieces of one item), wave
    1's behind a stretch of one-item pieces where two items per float piece fit a run"""
    it, end = partition(total, nwaves)
    two = int((end - it).max()) >= 6
    w = 1 if two else 0
    head = [(_dec_one(k), 1) for k in range(int(it[w]))]
    k = 2 if two else 1
    head += [((dr.F32, 2, _dec_length(k, 2, 8), "f32_inf"), k), ((dr.S16, 1, 100, "s16"), 1),
             ((dr.F32, 1, 248, "f32_clean"), 1), ((dr.F64, 2, _dec_length(k, 2, 8), "f64_1e300"), k)]
    return head


@functools.lru_cache(maxsize=None)
def decode_case(total):
    nwaves = grid_waves("decode", total)
    recs = assemble(total, _dec_head(total, nwaves), _dec_one, _dec_many, [], DEC_CHUNK)
    for (fmt, ch, length, _), items in recs:
        assert length >= 1 and dec_items(ch, length) == items, (fmt, ch, length, items)
    quartet = [i for i, (s, _) in enumerate(recs) if s[3] != "pool"]
    assert [recs[i][0][3] for i in quartet] == list(DEC_VERDICT) and quartet == list(range(quartet[0], quartet[0] + 4))
    return _case("decode", total, recs, quartet=quartet)


@functools.lru_cache(maxsize=None)
def _dec_pool(fmt, ch, seed):
    longest = _dec_length(DEC_CHUNK if (fmt, ch) in DEC_SMALL else 256, min(2, ch), 0) if ch <= 2 else 256
    return dr.random_raw(np.random.default_rng(1000 * seed + 10 * fmt + ch), fmt, ch, longest)


@functools.lru_cache(maxsize=None)
def _dec_raw(spec, placement, seed):
    fmt, ch, length, source = spec
    if source == "pool":
        return _dec_pool(fmt, ch, seed)[:length * ch * dr.BYTES[fmt]]
    raw = dr.random_raw(np.random.default_rng(7000 + 10 * seed + DEC_VERDICT.index(source)), fmt, ch, length).copy()
    at = length * ch - 1 if placement == "last" else 0           # the clip's last sample / its first
    if seed == 0 and source == "f32_inf":
        raw.view(f32)[at] = np.inf
    if seed == 0 and source == "f64_1e300":
        raw.view(np.float64)[at] = 1e300
    raw.setflags(write=False)
    return raw


def decode_sources(c, placement, seed=0):
    """[(raw bytes, format, channels, sample_rate)] of the call; seed 0: the case, any other: clips of the same sizes and formats with
    other values and no non-finite sample (what lies in the extents before the call)"""
    return [(_dec_raw(s, placement, seed), s[0], s[1], 48000.0) for s in c["specs"]]


@functools.lru_cache(maxsize=None)
def decode_want(spec, placement):
    """(the words of the clip's extent, the finite flag) from the restatement"""
    planar = dr.decode(_dec_raw(spec, placement, 0), spec[0], spec[1])
    ext = dr.extent(planar)
    ext.setflags(write=False)
    return ext, dr.finite(planar)


def decode_stage_bytes(c):
    return int(sum((length * ch * dr.BYTES[fmt] + 15) & ~15 for fmt, ch, length, _ in c["specs"]))


def decode_facts(c):
    q0, q3 = c["quartet"][0], c["quartet"][-1]
    first, last = int(c["bases"][q0]), int(c["bases"][q3] + c["items"][q3] - 1)
    it, _ = partition(c["total"], c["nwaves"])
    return dict(quartet_runs=run_of(c["total"], c["nwaves"], last) - run_of(c["total"], c["nwaves"], first) + 1,
                quartet_starts_a_run=bool(it[run_of(c["total"], c["nwaves"], first)] == first),
                poison_behind_a_clean_piece=any(run_of(c["total"], c["nwaves"], int(c["bases"][i] + (c["items"][i] - 1 if p == "last" else 0)))
                                                == run_of(c["total"], c["nwaves"], int(c["bases"][i]) - 1)
                                                for i in (q0, q3) if c["bases"][i] > 0 for p in PLACEMENTS))


# ---- limits --------------------------------------------------------------------------------------------------------------------------
def limits(c):
    """the documented limits of the call the case makes, asserted; returns the figure that is nearest to its limit"""
    if c["service"] == "onset":
        assert c["items"].max() <= header_value("onset", "MAX_HOPS") and c["total"] <= header_value("onset", "MAX_CALL_HOPS")
        assert all(hop in ON_HOPS and header_value("onset", "HOP_MIN") <= hop <= header_value("onset", "HOP_MAX") for _, _, _, hop in c["specs"])
        return c["total"]
    if c["service"] == "overview":
        columns = sum(s[1] for s in c["specs"])
        assert max(s[1] for s in c["specs"]) <= header_value("overview", "MAX_COLUMNS") and columns <= header_value("overview", "MAX_CALL_COLUMNS")
        return columns
    staged = decode_stage_bytes(c)
    assert staged <= header_value("decode", "STAGE_DEFAULT")       # one pass, so one decode launch
    assert max(s[1] for s in c["specs"]) <= header_value("decode", "MAX_CHANNELS")
    return staged
