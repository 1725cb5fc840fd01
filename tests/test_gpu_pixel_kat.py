"""Known-answer tests of the pixel stage: the nine kernels of grayshift_amd/csrc/device/pixel.hpp --
gs_combine_kernel, gs_accumulate_kernel, gs_views_order_kernel, gs_views_accumulate_kernel and the
batch rounds' init, params, combine, fold and resolve kernels -- launched as they are through the
test-only harness (tests/hip/kat_device.hip, kat_pixel_*) on hand-built parameter blocks.

References: oracle.sample_fold (the oracle's own Camera::sample loop over given sample colours) for the
fold and the stop test; tests/pixel_cases.py's numpy f64 restatement for what is layout and scheduling.
tests/test_pixel_cases_host.py asserts on the references alone that the cases reach the edges.

Every comparison is bit for bit -- f64 and f32 through their integer views, a NaN matched by position,
bytes and words by equality: every operation involved is + - * /, sqrt, a cast, color_byte or sat_u64,
correctly rounded and libm-free.  Every buffer a kernel can write goes up holding a poison pattern, so
what a kernel must leave alone is compared too.  Active lists filled through atomics are compared as
sorted sets with their counts, and by the within-wave rule (pixel_cases.within_wave_rule)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import pixel_cases as X

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIST_POISON = 0xFFFFFFF1
WORD_POISON = 0x7A7A7A7A


class KLayout(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("world", C.c_int32),
                ("rank", C.c_int32), ("slots", C.c_uint32), ("n_pos", C.c_uint32), ("direct", C.c_uint32),
                ("bs", C.c_uint32), ("chunk", C.c_uint32), ("cpp", C.c_uint32), ("fine_px", C.c_uint32),
                ("fine_base", C.c_uint32), ("max_samples", C.c_uint32), ("cap", C.c_uint32),
                ("confidence", C.c_double), ("tolerance", C.c_double), ("order", C.c_void_p), ("out", C.c_void_p),
                ("out8", C.c_void_p), ("n_out", C.c_uint64)]


def ptr(a):
    return None if a is None else a.ctypes.data


def _ok(rc):
    """A harness call's status: after a HIP error nothing more is launched."""
    if rc == -1:
        pytest.exit("a harness kernel failed (status %d): no further launches" % rc, returncode=3)
    assert rc == 0, "the harness refused a well-formed case (status %d)" % rc


@pytest.fixture(scope="module")
def kat(built):
    lib = C.CDLL(os.path.join(HERE, "hip", "libkat_device.so"))
    P, I, U, Q = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    LP = C.POINTER(KLayout)
    for f, args in {"kat_pixel_layout_bytes": [], "kat_pixel_claim_consts": [I],
                    "kat_pixel_combine": [LP, U, P, Q],
                    "kat_pixel_accumulate": [LP, U, P, Q, P, P, P, P, P],
                    "kat_pixel_views_order": [LP, P, P, U, U, P],
                    "kat_pixel_views_accumulate": [LP, P, P, U, U, P, Q, P, P],
                    "kat_pixel_round_init": [LP, U, P, P],
                    "kat_pixel_round_params": [P, P, P, P],
                    "kat_pixel_round_step": [LP, I, U, U, P, U, U, U, P, Q, P, P, P, P, P],
                    "kat_pixel_round_resolve": [LP, P, P, P, P, P]}.items():
        getattr(lib, f).argtypes = args
        getattr(lib, f).restype = I
    lib.kat_pixel_accum_blocks.argtypes = [U]
    lib.kat_pixel_accum_blocks.restype = U
    lib.kat_pixel_stopped_bit.restype = U
    assert lib.kat_pixel_layout_bytes() == C.sizeof(KLayout)
    assert [lib.kat_pixel_claim_consts(k) for k in range(3)] == [X.CLAIM_DIV, X.CLAIM_FINE, X.WHOLE_MAX_BATCH]
    assert lib.kat_pixel_stopped_bit() == X.STOPPED
    for cap in (0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1, 528384):
        assert lib.kat_pixel_accum_blocks(cap) == X.accum_blocks(cap)
    return lib


def klayout(lay, out, out8, bs=1, ch=None, max_samples=0, conf=0.0, tol=0.0):
    """The harness's layout record; keeps the arrays it points to alive."""
    k = KLayout(lay.W, lay.H, lay.tw, lay.th, lay.world, lay.rank, lay.slots, lay.n_pos, lay.direct, bs,
                ch.chunk if ch else 0, ch.cpp if ch else 1, ch.fine_px if ch else lay.cap, ch.fine_base if ch else 0,
                max_samples, lay.cap, conf, tol, ptr(lay.order), ptr(out), ptr(out8), lay.n_out)
    k._keep = (lay.order, out, out8)
    return k


outsel = X.outsel
layouts_of = X.layouts_of  # (the host test asserts on the very layouts these tests run)
chunkings = X.chunkings


def check(name, got, want):
    if want is None:
        assert got is None
        return
    if not X.same_bits(got, want):
        d = X.where_differs(got, want)
        i = tuple(d[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (name, len(d), got.size, i, got[i], want[i]))


FT = [(fi, ti) for fi in range(3) for ti in range(3)]
FT_IDS = ["%dx%d-t%dx%d" % (X.FRAMES[f] + X.TILES[t]) for f, t in FT]


# ------------------------------------------------------------------ the harness refuses malformed cases
def test_harness_refuses_malformed_cases(kat):
    lay = X.layout(21, 13, 8, 8, 1, 0, "holes", 0, seed=3)
    ch = X.Chunking(lay.cap, 4, 2, 2, lay.cap)
    part = X.make_partial(ch, 1)
    out, out8 = X.poison_outputs(lay)

    def combine(l, p=part, o=out):
        return kat.kat_pixel_combine(C.byref(klayout(l, o, out8, ch.bs, ch)), 2, ptr(p), len(p))

    _ok(combine(lay))
    bad = X.Layout(21, 13, 8, 8, 1, 0, lay.order.copy(), 0)
    bad.order[2] = lay.n_tiles  # not a tile of the frame
    assert combine(bad) == -2
    bad.order[2] = -2
    assert combine(bad) == -2
    short = X.Layout(21, 13, 8, 8, 1, 0, lay.order[:-1].copy(), 0, slots=lay.slots)  # the last slot has no position
    assert combine(short) == -2
    assert combine(lay, p=part[:-1]) == -2  # sums past the buffer
    wrong = klayout(lay, out, out8, ch.bs, ch)
    wrong.n_out -= 1
    assert kat.kat_pixel_combine(C.byref(wrong), 2, ptr(part), len(part)) == -2
    wrong = klayout(lay, out, out8, ch.bs, ch)
    wrong.cap += lay.tile_px  # the per-pixel arrays sized for another capacity than the layout's
    assert kat.kat_pixel_combine(C.byref(wrong), 2, ptr(part), len(part)) == -2
    # views: tile_h must divide a view's rows; a vorder entry must be a tile
    vl = X.Layout(24, 48, 8, 8, 1, 0, None, 0, slots=18)
    vs = np.array([[0, 1], [8, 0], [0, 1]], dtype=np.uint32)
    dst = np.full(vl.n_pos, -7, dtype=np.int32)
    o, o8 = X.poison_outputs(vl)
    assert kat.kat_pixel_views_order(C.byref(klayout(vl, o, o8, 4)), None, ptr(vs), 3, 16, ptr(dst)) == 0
    assert kat.kat_pixel_views_order(C.byref(klayout(vl, o, o8, 4)), None, ptr(vs), 4, 12, ptr(dst)) == -2
    vo = np.arange(vl.n_pos, dtype=np.int32)
    vo[5] = 18
    assert kat.kat_pixel_views_order(C.byref(klayout(vl, o, o8, 4)), ptr(vo), ptr(vs), 3, 16, ptr(dst)) == -2
    # rounds: an active entry past the capacity or on a padding slot; a segment past the list
    real, _ = X.out_index(lay)
    good = np.flatnonzero(real)[:10].astype(np.uint32)
    part2 = np.zeros(10 * 3)
    ps = np.zeros((lay.cap, 5))
    nxt = np.zeros(lay.cap, dtype=np.uint32)

    def step(active, seg_base, seg_n):
        cnt = np.zeros(1, dtype=np.uint32)
        return kat.kat_pixel_round_step(C.byref(klayout(lay, out, out8, 1, None, 5, 1.0, 0.1)), 0, 0, 1, ptr(active),
                                        len(active), seg_base, seg_n, ptr(part2), len(part2), ptr(ps), None, ptr(nxt),
                                        ptr(cnt), None)

    _ok(step(good, 2, 8))
    assert step(good, 3, 8) == -2
    a = good.copy()
    a[4] = lay.cap
    assert step(a, 0, 10) == -2
    a[4] = np.flatnonzero(~real)[0]
    assert step(a, 0, 10) == -2


# ------------------------------------------------------------------ gs_combine_kernel
@pytest.mark.parametrize("fi,ti", FT, ids=FT_IDS)
def test_combine_shared_layouts(kat, fi, ti):
    for n, lay, sel in layouts_of(fi, ti):
        chs = chunkings(lay.cap, lay.tile_px)
        ch = chs[(7 * n + fi + 3 * ti) % len(chs)]
        part = X.make_partial(ch, 1000 * fi + 100 * ti + n)
        wo, wo8 = outsel(sel)
        out, out8 = X.poison_outputs(lay, wo, wo8)
        grid = (1, 3, X.accum_blocks(lay.cap))[n % 3]
        _ok(kat.kat_pixel_combine(C.byref(klayout(lay, out, out8, ch.bs, ch)), grid, ptr(part), len(part)))
        eo, eo8 = X.combine_ref(lay, ch, part, wo, wo8)
        check("%s out" % lay.key(), out, eo)
        check("%s out8" % lay.key(), out8, eo8)


@pytest.mark.parametrize("specials", [False, True], ids=["magnitudes", "specials"])
def test_combine_every_chunking(kat, specials):
    for li, lay in enumerate((X.layout(80, 45, 16, 4, 1, 0, "perm", 0, seed=5), X.layout(80, 45, 8, 8, 3, 2, "holes", 1, seed=6))):
        for ci, ch in enumerate(chunkings(lay.cap, lay.tile_px)):
            part = X.make_partial(ch, 50 * li + ci, specials=specials)
            out, out8 = X.poison_outputs(lay)
            _ok(kat.kat_pixel_combine(C.byref(klayout(lay, out, out8, ch.bs, ch)), (1, 5)[ci % 2], ptr(part), len(part)))
            eo, eo8 = X.combine_ref(lay, ch, part)
            check("chunking %d out" % ci, out, eo)
            check("chunking %d out8" % ci, out8, eo8)


# ------------------------------------------------------------------ gs_accumulate_kernel
def run_accumulate(kat, lay, ch, seed, wo, wo8, specials, with_delta=True, n_pass=3):
    """n_pass chained passes; accum, the outputs and delta[b] compared after each.  `specials`:
    pixel_cases.accumulate_parts -- a block's change is compared as a number only while no NaN or inf has
    reached one of its pixels (a NaN matches any NaN), so every layout also runs passes without them."""
    blocks = X.accum_blocks(lay.cap)
    parts = X.accumulate_parts(ch, seed, n_pass, specials)
    acc0 = np.zeros((lay.cap, 3))
    acc_out = np.full((n_pass, lay.cap, 3), 1.25)
    out, out8 = X.poison_outputs(lay, wo, wo8)
    out_all = None if out is None else np.zeros((n_pass,) + out.shape, dtype=np.float32)
    out8_all = None if out8 is None else np.zeros((n_pass,) + out8.shape, dtype=np.uint8)
    delta = np.full((n_pass, blocks), -3.0) if with_delta else None
    _ok(kat.kat_pixel_accumulate(C.byref(klayout(lay, out, out8, ch.bs, ch)), n_pass, ptr(parts), parts.shape[1],
                                 ptr(acc0), ptr(acc_out), ptr(out_all), ptr(out8_all), ptr(delta)))
    acc = acc0
    for p in range(n_pass):
        acc, eo, eo8, ed = X.accumulate_ref(lay, ch, parts[p], acc, p * ch.bs, wo, wo8)
        check("%s pass %d accum" % (lay.key(), p), acc_out[p], acc)
        check("%s pass %d out" % (lay.key(), p), None if out_all is None else out_all[p], eo)
        check("%s pass %d out8" % (lay.key(), p), None if out8_all is None else out8_all[p], eo8)
        if with_delta:
            check("%s pass %d delta" % (lay.key(), p), delta[p], ed)


@pytest.mark.parametrize("name", list(X.ACC_LAYOUTS))
def test_accumulate_three_passes(kat, name):
    """Three chained passes; 129 tiles of 64 x 64 pass GS_ACCUM_MAX_BLOCKS * 256, so the grid-stride loop runs.
    Every capacity runs clean sums -- test_pixel_cases_host.py asserts that every block's expected change is
    then a finite non-zero number in every pass -- and the small ones run sums with specials too."""
    for lay, ch, seed, specials, with_delta in X.accumulate_named_cases(name):
        run_accumulate(kat, lay, ch, seed, True, with_delta, specials, with_delta=with_delta)  # (delta null: out alone)


@pytest.mark.parametrize("fi,ti", FT, ids=FT_IDS)
def test_accumulate_shared_layouts(kat, fi, ti):
    for n, lay, sel in layouts_of(fi, ti):
        ch, seed = X.accumulate_shared_case(fi, ti, n, lay)
        wo, wo8 = outsel(sel)
        run_accumulate(kat, lay, ch, seed, wo, wo8, "last")  # (passes 0 and 1 clean: their changes are numbers)


# ------------------------------------------------------------------ the views kernels
VIEW_SETS = (((1, 0, 1), (0, 8, 0)), ((0, 1, 1), (16, 0, 8)))
VIEW_FRAMES = {"t8x8": (24, 16, 8, 8), "t16x4": (24, 16, 16, 4), "t64x64": (70, 64, 64, 64),
               "t8x8-300tiles": (200, 32, 8, 8)}  # (the last: more than 256 positions, two blocks of the order kernel)


def view_orders(lay, seed):
    rng = np.random.default_rng(seed)
    perm = np.full(lay.n_pos, -1, dtype=np.int32)
    perm[rng.permutation(lay.n_pos)[:lay.n_tiles]] = rng.permutation(lay.n_tiles)
    holes = perm.copy()
    holes[rng.choice(np.flatnonzero(holes >= 0), max(1, lay.n_tiles // 4), replace=False)] = -1
    return (None, perm, holes)


@pytest.mark.parametrize("frame", list(VIEW_FRAMES))
def test_views_order_and_accumulate(kat, frame):
    W, vh, tw, th = VIEW_FRAMES[frame]
    V, n = 3, 0
    for (world, rank) in X.RANKS:
        for direct in (0, 1):
            base = X.Layout(W, V * vh, tw, th, world, rank, None, direct)
            lay = X.Layout(W, V * vh, tw, th, world, rank, None, direct, slots=base.slots + 1)
            for vi, vorder in enumerate(view_orders(lay, 40 + n)):
                for (selected, before) in VIEW_SETS:
                    n += 1
                    vs = np.array(list(zip(before, selected)), dtype=np.uint32)
                    wo, wo8 = outsel(n)
                    # the pass's order
                    dst = np.full(lay.n_pos, -7, dtype=np.int32)
                    o, o8 = X.poison_outputs(lay, wo, wo8)
                    _ok(kat.kat_pixel_views_order(C.byref(klayout(lay, o, o8, 8)), ptr(vorder), ptr(vs), V, vh, ptr(dst)))
                    check("views order", dst, X.views_order_ref(lay, vorder, vs, vh))
                    # the pass's accumulate
                    ch = X.Chunking(lay.cap, 8, 2, 4, (0, (lay.slots // 2) * lay.tile_px, lay.cap)[n % 3])
                    part = X.make_partial(ch, 300 + n, specials=False)
                    rng = np.random.default_rng(n)
                    acc0 = rng.uniform(-4.0, 9.0, (lay.cap, 3)) * 10.0 ** rng.integers(-6, 4, (lay.cap, 1))
                    acc = acc0.copy()
                    vdelta = np.full(lay.slots, -3.0)
                    _ok(kat.kat_pixel_views_accumulate(C.byref(klayout(lay, o, o8, ch.bs, ch)), ptr(vorder), ptr(vs), V, vh,
                                                       ptr(part), len(part), ptr(acc), ptr(vdelta) if n % 4 else None))
                    ea, eo, eo8, ev = X.views_accumulate_ref(lay, ch, vorder, vs, vh, part, acc0, wo, wo8)
                    check("views accum", acc, ea)
                    check("views out", o, eo)
                    check("views out8", o8, eo8)
                    if n % 4:
                        check("views vdelta", vdelta, ev)
                    # an unselected view's sums are untouched, bit for bit, and resolve to sums / before or 0.0
                    real, pi, pj = X.packed_pixel(lay, vorder)
                    unsel = real & (vs[np.where(real, pj // vh, 0), 1] == 0)
                    assert (X.bits(acc[unsel]) == X.bits(acc0[unsel])).all()
                    zero_view = unsel & (vs[np.where(real, pj // vh, 0), 0] == 0)
                    if o is not None and zero_view.any():
                        _, oi = X.out_index(lay, vorder)
                        assert (X.bits(o[oi[zero_view]]) == 0).all()  # +0.0, not 0 / 0


# ------------------------------------------------------------------ gs_round_init_kernel
@pytest.mark.parametrize("grid", [1, 8])
@pytest.mark.parametrize("fi,ti", FT, ids=FT_IDS)
def test_round_init(kat, fi, ti, grid):
    for n, lay, sel in layouts_of(fi, ti):
        wo, wo8 = outsel(sel)
        out, out8 = X.poison_outputs(lay, wo, wo8)
        active = np.full(lay.cap, LIST_POISON, dtype=np.uint32)
        count = np.zeros(1, dtype=np.uint32)
        _ok(kat.kat_pixel_round_init(C.byref(klayout(lay, out, out8, 4)), grid, ptr(active), ptr(count)))
        real, _ = X.out_index(lay)
        want = np.flatnonzero(real).astype(np.uint32)
        assert count[0] == len(want), lay.key()
        got = active[:len(want)]
        assert (np.sort(got) == want).all() and (active[len(want):] == LIST_POISON).all(), lay.key()
        assert X.within_wave_rule(np.arange(lay.cap), got), lay.key()
        # padding outputs zeroed (packed), nothing else written
        eo, eo8 = X.expected_outputs(lay, np.zeros((lay.cap, 3)), np.zeros(lay.cap, dtype=bool), want_out=wo, want_out8=wo8)
        check("init out", out, eo)
        check("init out8", out8, eo8)


# ------------------------------------------------------------------ gs_round_params_kernel
@pytest.mark.parametrize("name,a", X.params_table(), ids=[n for n, _ in X.params_table()])
def test_round_params(kat, name, a):
    want, hint_after, _ = X.round_params_ref(**a)
    cnt = a["counters"]
    inp = np.array([a["round"], a["seg"], a["seg_px"], a["chunk_req"] & X.U32, a["whole_mode"] & X.U32, a["bs"], a["lanes"],
                    a["waves"], a["capacity"], a["n_act"], 0 if cnt is None else 1, WORD_POISON], dtype=np.uint32)
    counters = np.array(cnt if cnt is not None else (0, 0), dtype=np.uint64)
    hint = np.array(a["hint"], dtype=np.uint64)
    out = np.full(24, 0x55555555, dtype=np.uint32)
    _ok(kat.kat_pixel_round_params(ptr(inp), ptr(counters), ptr(hint), ptr(out)))
    got = dict(zip(X.PARAMS_FIELDS, (int(v) for v in out)))
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert tuple(int(v) for v in hint) == tuple(hint_after)


# ------------------------------------------------------------------ gs_round_combine_kernel, gs_round_fold_kernel
STEP_LAYOUTS = (lambda: X.layout(80, 45, 16, 4, 1, 0, "holes", 0, seed=9), lambda: X.layout(80, 45, 8, 8, 1, 0, "perm", 1, seed=8))


def run_step(kat, lay, st, rnd, fold, seg_n, seg_base, grid, sel, seed, counters=True, whole=False):
    """One launch of round `rnd` over a shuffled active list; everything it may write is compared.
    counters: with the launch's counters (else null).  whole: the combine of a whole-batch round
    (per_sample 0), which must write nothing at all."""
    rng = np.random.default_rng(seed)
    real, oi = X.out_index(lay)
    active_streams, state = X.round_inputs(st, rnd)
    assert len(active_streams) >= seg_base + seg_n, (st.name, rnd, len(active_streams), seg_base + seg_n)
    pix_of = rng.permutation(np.flatnonzero(real))[:st.n].astype(np.uint32)  # stream -> packed pixel
    assert len(pix_of) == st.n
    listed = rng.permutation(active_streams)
    active = pix_of[listed]
    seg = listed[seg_base:seg_base + seg_n]
    part = X.round_partial(st, rnd, seg)
    if len(part) == 0:
        part = np.zeros(3)
    wo, wo8 = outsel(sel)
    out, out8 = X.poison_outputs(lay, wo, wo8)
    pstate = np.full((lay.cap, 5), X.NAN_POISON)  # round 0 runs over poison: the state must not be read
    pbatches = np.full(lay.cap, WORD_POISON, dtype=np.uint32)
    if rnd:
        pstate[active] = state[listed]
        pbatches[active] = rnd
    pstate0, pbatches0 = pstate.copy(), pbatches.copy()
    c0 = 5
    nxt = np.full(lay.cap, LIST_POISON, dtype=np.uint32)
    count = np.array([c0], dtype=np.uint32)
    pix = np.array([1000], dtype=np.uint64) if counters else None
    assert not (whole and fold)
    _ok(kat.kat_pixel_round_step(C.byref(klayout(lay, out, out8, st.bs, None, st.max_samples, st.conf, st.tol)),
                                 2 if whole else fold, rnd, grid, ptr(active), len(active), seg_base, seg_n, ptr(part),
                                 len(part), ptr(pstate), ptr(pbatches) if fold else None, ptr(nxt), ptr(count), ptr(pix)))
    stops, sums, colour = X.round_expect(st, rnd, seg)
    tag = "%s %s round %d %s" % (lay.key(), st.name, rnd, "fold" if fold else "combine")
    if whole:  # the lanes took the stop test: nothing is the combine's to write
        eo, eo8 = X.poison_outputs(lay, wo, wo8)
        assert count[0] == c0 and (pix is None or pix[0] == 1000) and (nxt == LIST_POISON).all(), tag
        for name, got, want in (("pstate", pstate, pstate0), ("pbatches", pbatches, pbatches0), ("out", out, eo), ("out8", out8, eo8)):
            check(tag + " whole-batch round: " + name, got, want)
        return stops
    # the next list: contents, count, the within-wave rule, nothing else written
    go = pix_of[seg[~stops]]
    assert count[0] == c0 + len(go), tag
    got = nxt[c0:c0 + len(go)]
    assert (np.sort(got) == np.sort(go)).all(), tag
    assert (nxt[:c0] == LIST_POISON).all() and (nxt[c0 + len(go):] == LIST_POISON).all(), tag
    assert X.within_wave_rule(active[seg_base:seg_base + seg_n], got), tag
    assert pix is None or pix[0] == 1000 + int(stops.sum()), tag
    # the state: continuing pixels hold the sums; a stopped one keeps what it had (combine) or holds its
    # final sums with the stopped word (fold); everything outside the segment is untouched
    want_state, want_b = pstate0.copy(), pbatches0.copy()
    keep = np.ones(len(seg), dtype=bool) if fold else ~stops
    want_state[pix_of[seg[keep]]] = sums[keep]
    if fold:
        want_b[pix_of[seg]] = (rnd + 1) | np.where(stops, X.STOPPED, 0).astype(np.uint32)
    check(tag + " pstate", pstate, want_state)
    check(tag + " pbatches", pbatches, want_b)
    # the outputs: combine writes a stopped pixel's colour at its index, and nothing else
    eo, eo8 = X.poison_outputs(lay, wo, wo8)
    if not fold:
        at = oi[pix_of[seg[stops]]]
        if eo is not None:
            eo[at] = X.to_f32(colour[stops])
        if eo8 is not None:
            eo8[at] = X.color_byte(colour[stops])
    check(tag + " out", out, eo)
    check(tag + " out8", out8, eo8)
    return stops


@pytest.mark.parametrize("bs", [1, 2, 3, 16, 257])
@pytest.mark.parametrize("seg_n", [1, 63, 64, 65, 1000])
def test_round_step_shapes(kat, seg_n, bs):
    n = seg_n + 40 + (600 if seg_n == 1000 else 200)
    st = X.mixed_case(n, bs, 3, 100 * seg_n + bs)
    k = 0
    for rnd in (0, 1):
        active, _ = X.round_inputs(st, rnd)
        sn = min(seg_n, len(active) - 7)
        assert sn == seg_n or (rnd == 1 and seg_n == 1000 and sn > 500), (len(active), seg_n)
        for fold in (0, 1):
            lay = STEP_LAYOUTS[k % 2]()
            run_step(kat, lay, st, rnd, fold, sn, 7, (1, 2, 16)[k % 3], k, 900 + k)
            k += 1


@pytest.mark.parametrize("fi,ti", FT, ids=FT_IDS)
def test_round_step_shared_layouts(kat, fi, ti):
    """gs_round_combine_kernel places a stopped pixel's colour through packed_pixel in `direct` mode: the
    shared layout cases, rounds 0 and 1 of a small mixed stream on up to 40 of the rank's real pixels, the
    colours at the image index and the poison everywhere else.  The fold kernel runs on every third layout
    (it takes no index but the packed one); some launches run without counters."""
    ran = stopped = 0
    for n, lay, sel in layouts_of(fi, ti):
        real, _ = X.out_index(lay)
        if not real.any():  # (a rank that owns no tile of a one-tile frame: no pixel can be active)
            continue
        st = X.pool_streams(min(int(real.sum()), 40), 7 * n + fi + 3 * ti, short=n % 2 == 1)
        for rnd in (0, 1):
            active, _ = X.round_inputs(st, rnd)
            if len(active) == 0:
                break
            base = min(3, len(active) - 1)
            for fold in ((0, 1) if n % 3 == 0 else (0,)):
                stops = run_step(kat, lay, st, rnd, fold, len(active) - base, base, (1, 2)[n % 2], sel, 1700 + n,
                                 counters=(n + rnd) % 4 != 0)
                ran += 1
                stopped += int(stops.sum())
    assert ran >= 18 and stopped > 0  # (test_pixel_cases_host.py: which layouts have real pixels, and how many stop)


def test_round_combine_leaves_whole_batch_rounds_alone(kat):
    st = X.mixed_case(300, 4, 3, 77)
    for k, rnd in enumerate((0, 1)):
        active, _ = X.round_inputs(st, rnd)
        run_step(kat, STEP_LAYOUTS[k](), st, rnd, 0, len(active) - 5, 5, 2, k, 2100 + k, whole=True)


_FAMILIES = []


def families():
    """pixel_cases.family_cases(), built once (the oracle folds every stream)."""
    if not _FAMILIES:
        _FAMILIES.extend(X.family_cases())
    return _FAMILIES


@pytest.mark.parametrize("fam", ["thr", "constant_tol0", "black", "max_kbs_minus_1", "max_kbs", "max_zero", "max_u32max",
                                 "nan_inf", "negative", "bs1"])
def test_round_step_families(kat, fam):
    k = 0
    for st in families():
        if not (st.name == fam or (fam == "thr" and st.name.startswith("thr_"))):
            continue
        for rnd in range(st.nb):
            active, _ = X.round_inputs(st, rnd)
            if len(active) == 0:
                break
            for fold in (0, 1):
                lay = STEP_LAYOUTS[k % 2]()
                base = min(3, len(active) - 1)
                run_step(kat, lay, st, rnd, fold, len(active) - base, base, (1, 4)[k % 2], k, 1300 + k)
                k += 1
    assert k > 0


@pytest.mark.parametrize("li", [0, 1], ids=["packed-holes", "direct-perm"])
@pytest.mark.parametrize("fold", [0, 1], ids=["combine", "fold"])
def test_round_chain(kat, fold, li):
    """Rounds 0..R fed back through the lists, two segments a round: every pixel's batches taken, final
    sums and colour equal oracle.sample_fold of its whole stream."""
    st = X.mixed_case(1000, 4, 12, 4242)
    f = st.fold()
    lay = STEP_LAYOUTS[li]()
    real, oi = X.out_index(lay)
    rng = np.random.default_rng(5)
    pix_of = rng.permutation(np.flatnonzero(real))[:st.n].astype(np.uint32)
    stream_of = {int(p): i for i, p in enumerate(pix_of)}
    out, out8 = X.poison_outputs(lay)
    pstate = np.full((lay.cap, 5), X.NAN_POISON)
    pbatches = np.full(lay.cap, X.STOPPED, dtype=np.uint32)  # (padding and unused pixels: never active)
    pbatches[pix_of] = 0
    kl = klayout(lay, out, out8, st.bs, None, st.max_samples, st.conf, st.tol)
    active = rng.permutation(pix_of)
    left = np.zeros(st.n, dtype=np.int64)
    pix = np.array([0], dtype=np.uint64)
    seg_px = 600
    for rnd in range(13):
        if len(active) == 0:
            break
        assert rnd < st.nb
        nxt = np.full(lay.cap, LIST_POISON, dtype=np.uint32)
        count = np.zeros(1, dtype=np.uint32)
        streams = np.array([stream_of[int(p)] for p in active])
        for base in range(0, len(active), seg_px):
            sn = min(seg_px, len(active) - base)
            part = X.round_partial(st, rnd, streams[base:base + sn])
            _ok(kat.kat_pixel_round_step(C.byref(kl), fold, rnd, (3, 1)[rnd % 2], ptr(active), len(active), base, sn,
                                         ptr(part), len(part), ptr(pstate), ptr(pbatches) if fold else None, ptr(nxt),
                                         ptr(count), ptr(pix)))
        left[streams] = rnd + 1
        assert count[0] == int((f["batches"] > rnd + 1).sum()), rnd
        active = nxt[:count[0]].copy()
    assert len(active) == 0 and pix[0] == st.n
    assert (left == f["batches"]).all()
    assert set(f["reason"].tolist()) == {1, 2}
    if fold:
        assert (pbatches[pix_of] == (f["batches"] | X.STOPPED)).all()
        check("chain sums", pstate[pix_of], f["sums"][np.arange(st.n), f["batches"] - 1])
        ms = np.full(lay.cap, WORD_POISON, dtype=np.uint32)
        me = np.full(lay.cap, -7.5, dtype=np.float32)
        summary = np.zeros(4, dtype=np.uint64)
        _ok(kat.kat_pixel_round_resolve(C.byref(kl), ptr(pstate), ptr(pbatches), ptr(ms), ptr(me), ptr(summary)))
        assert (ms[pix_of] == f["batches"] * st.bs).all()
    check("chain colour", out[oi[pix_of]], X.to_f32(f["color"]))
    check("chain bytes", out8[oi[pix_of]], X.color_byte(f["color"]))


# ------------------------------------------------------------------ gs_round_resolve_kernel
def resolve_state(lay, bs, seed):
    """Hand-built sums and batch words: ordinary pixels; a mean of 0; a negative variance; one round of a
    one-sample batch; words whose samples pass 2^32 - 1; a pixel never sampled."""
    rng = np.random.default_rng(seed)
    cap = lay.cap
    nb = rng.integers(1, 9, cap)
    word = (nb | np.where(rng.random(cap) < 0.5, X.STOPPED, 0)).astype(np.uint32)
    n = (nb * bs).astype(np.float64)
    mean = rng.uniform(0.05, 3.0, cap)
    ps = np.empty((cap, 5))
    ps[:, :3] = rng.uniform(0.0, 2.0, (cap, 3)) * n[:, None]
    ps[:, 3] = mean * n
    ps[:, 4] = (mean * mean + rng.uniform(0.0, 0.5, cap)) * n
    k = rng.permutation(cap)
    q = max(1, cap // 16)
    ps[k[:q], 3] = 0.0                       # mean 0: x / 0
    ps[k[q:2 * q], 4] = 0.5 * ps[k[q:2 * q], 3] ** 2 / n[k[q:2 * q]]  # lsq < lsum^2 / n: sqrt of a negative
    word[k[2 * q:3 * q]] = 0x7FFFFFFF - rng.integers(0, 3, q).astype(np.uint32)  # word * bs saturates (bs > 2)
    word[k[3 * q:4 * q]] = 0                 # never sampled: 0 / 0
    if bs == 1:
        word[k[4 * q:5 * q]] = 1             # one round of one sample: 1 / 0 * 0
    return ps, word


@pytest.mark.parametrize("bs", [1, 16])
@pytest.mark.parametrize("fi,ti", FT, ids=FT_IDS)
def test_round_resolve(kat, fi, ti, bs):
    for n, lay, sel in layouts_of(fi, ti):
        if n % 2 != (bs == 1):
            continue
        wo, wo8 = outsel(sel)
        out, out8 = X.poison_outputs(lay, wo, wo8)
        ps, word = resolve_state(lay, bs, 10 * n + fi + ti)
        maps = (n // 3) % 3 != 0  # (n % 3 is the out / out8 selection: every selection runs with and without the maps)
        ms = np.full(lay.cap, WORD_POISON, dtype=np.uint32) if maps else None
        me = np.full(lay.cap, -7.5, dtype=np.float32) if maps else None
        summary = np.zeros(4, dtype=np.uint64) if n % 5 else None
        _ok(kat.kat_pixel_round_resolve(C.byref(klayout(lay, out, out8, bs, None, 0, X.CONF, 0.0)), ptr(ps), ptr(word),
                                        ptr(ms), ptr(me), ptr(summary)))
        eo, eo8, ems, eme, esum = X.resolve_ref(lay, bs, X.CONF, ps, word, wo, wo8)
        check("resolve out", out, eo)
        check("resolve out8", out8, eo8)
        if maps:
            check("map_samples", ms, ems)
            check("map_error", me, eme)
        if summary is not None:
            assert tuple(int(v) for v in summary) == esum + (0,), lay.key()
