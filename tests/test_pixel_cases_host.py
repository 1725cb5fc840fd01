"""Conditions on the pixel-stage cases (tests/pixel_cases.py), asserted on the references alone -- the
oracle's sample_fold and the numpy restatement -- so that a green tests/test_gpu_pixel_kat.py means
something: the threshold and constant-colour cases fall on both sides of the stop test, the fine path's
association shows in the bits, every stop reason, every branch of the item-size rule and both selection
states of a view occur.  The vectorised restatement is also held against a scalar transcription, thread
by thread, on small cases.  No GPU needed."""
import numpy as np
import pytest

import oracle

from tests import pixel_cases as X


# ------------------------------------------------------------------ the restatement against a scalar transcription
def scalar_packed_pixel(lay, k):
    slot, w = divmod(k, lay.tile_px)
    pos = lay.rank + slot * lay.world
    tile = pos if lay.order is None else int(lay.order[pos])
    if tile == -1:
        return False, 0, 0
    pi = (tile % lay.tiles_x) * lay.tw + w % lay.tw
    pj = (tile // lay.tiles_x) * lay.th + w // lay.tw
    return pi < lay.W and pj < lay.H, pi, pj


def scalar_sums(ch, p, k, acc):
    r = list(acc)
    if k < ch.fine_px:
        for c in range(ch.cpp):
            for j in range(3):
                r[j] = r[j] + p[(c * ch.fine_px + k) * 3 + j]
    else:
        nf = ch.cap - ch.fine_px
        for s0 in range(0, ch.bs, ch.chunk):
            cs = [0.0, 0.0, 0.0]
            for s in range(s0, min(ch.bs, s0 + ch.chunk)):
                for j in range(3):
                    cs[j] = cs[j] + p[(ch.fine_base + s * nf + k - ch.fine_px) * 3 + j]
            for j in range(3):
                r[j] = r[j] + cs[j]
    return r


@pytest.mark.parametrize("kind", X.ORDERS)
@pytest.mark.parametrize("direct", [0, 1])
def test_accumulate_restatement_against_scalar_threads(kind, direct):
    lay = X.layout(21, 13, 8, 8, 3, 2, kind, direct, seed=4)
    ch = X.Chunking(lay.cap, 10, 2, 4, (lay.slots // 2) * lay.tile_px)
    part = [float(v) for v in X.make_partial(ch, 9, specials=False)]
    acc0 = np.random.default_rng(2).uniform(-3, 3, (lay.cap, 3))
    base = 20
    blocks = X.accum_blocks(lay.cap)
    change = [[0.0] * 256 for _ in range(blocks)]
    acc = acc0.copy()
    out = np.full((lay.n_out, 3), X.F32_POISON, dtype=np.float32)
    for b in range(blocks):
        for t in range(256):
            for k in range(b * 256 + t, lay.cap, blocks * 256):
                real, pi, pj = scalar_packed_pixel(lay, k)
                oi = pj * lay.W + pi if direct else k
                if not real:
                    if not direct:
                        out[oi] = 0.0
                    continue
                r0 = [float(v) for v in acc0[k]]
                r = scalar_sums(ch, part, k, r0)
                acc[k] = r
                for j in range(3):
                    c = r[j] / float(base + ch.bs)
                    out[oi, j] = np.float32(c)
                    change[b][t] = change[b][t] + abs(c - r0[j] / float(base))
    delta = []
    for b in range(blocks):
        v = change[b]
        h = 128
        while h:
            for t in range(h):
                v[t] = v[t] + v[t + h]
            h >>= 1
        delta.append(v[0])
    ea, eo, eo8, ed = X.accumulate_ref(lay, ch, np.array(part), acc0, base)
    assert X.same_bits(ea, acc) and X.same_bits(eo, out) and X.same_bits(ed, np.array(delta))
    assert (eo8[eo != X.F32_POISON] != X.U8_POISON).any()


def test_packed_pixels_of_all_ranks_tile_the_frame():
    for (W, H) in X.FRAMES:
        for (tw, th) in X.TILES:
            for kind in X.ORDERS:
                order = X.make_order(W, H, tw, th, 3, kind, 5)
                seen = np.zeros(W * H, dtype=np.int64)
                for rank in range(3):
                    lay = X.Layout(W, H, tw, th, 3, rank, order, 1) if order is not None else X.layout(W, H, tw, th, 3, rank)
                    real, pi, pj = X.packed_pixel(lay)
                    np.add.at(seen, (pj * W + pi)[real], 1)
                    for k in (0, lay.cap // 2, lay.cap - 1):
                        assert scalar_packed_pixel(lay, k) [0] == real[k]
                assert (seen == 1).all(), (W, H, tw, th, kind)


def test_shared_layouts_reach_the_edges():
    lays = X.shared_layouts()
    assert len(lays) == 3 * 3 * 3 * 3 * 2
    pad = [(~X.packed_pixel(l)[0]).any() for l in lays]
    assert sum(pad) > len(lays) // 2
    assert any(l.order is not None and (l.order[l.rank::l.world] < 0).any() and l.direct for l in lays)  # empty slots with direct
    assert any(l.cap > l.W * l.H for l in lays) and any(l.tile_px < 256 for l in lays) and any(l.tile_px > 256 for l in lays)


def _expected_deltas(lay, ch, seed, n_pass, specials):
    parts = X.accumulate_parts(ch, seed, n_pass, specials)
    acc, out = np.zeros((lay.cap, 3)), []
    for p in range(n_pass):
        acc, _, _, d = X.accumulate_ref(lay, ch, parts[p], acc, p * ch.bs, want_out=False, want_out8=False)
        out.append(d)
    return out


def test_accumulate_named_capacities_compare_the_reduction():
    """At 64, 256 and 320 packed pixels (a partial block, exactly one, one and a quarter) the clean runs'
    expected change is a finite non-zero number in every block and every pass, with `direct` 0 and 1: a NaN
    there would match whatever the kernel reduced."""
    for name in ("cap64", "cap256", "cap320"):
        clean = [c for c in X.accumulate_named_cases(name) if c[3] == "none" and c[4]]
        assert sorted(c[0].direct for c in clean) == [0, 1]
        assert any(c[3] == "all" and c[4] for c in X.accumulate_named_cases(name))  # specials for accum and the outputs
        assert any(not c[4] for c in X.accumulate_named_cases(name))                # delta null
        for lay, ch, seed, specials, _ in clean:
            deltas = _expected_deltas(lay, ch, seed, 3, specials)
            assert len(deltas) == 3 and len(deltas[0]) == X.accum_blocks(lay.cap) == -(-lay.cap // 256)
            for p, d in enumerate(deltas):
                assert np.isfinite(d).all() and (d != 0.0).all(), (name, lay.direct, p, d)
            # ... and the passes' figures differ, so swapped sample counts or a stale `before` would show
            assert len({d.tobytes() for d in deltas}) == 3
    big = X.accumulate_named_cases("cap528384")
    assert [c[3] for c in big] == ["none"] and X.accum_blocks(big[0][0].cap) == X.ACCUM_MAX_BLOCKS < -(-big[0][0].cap // 256)


@pytest.mark.parametrize("fi", range(len(X.FRAMES)))
def test_accumulate_shared_layouts_compare_the_reduction(fi):
    """Every shared layout's passes 0 and 1 (no specials before the last pass): each block's expected change
    is finite, and non-zero exactly where the block holds a real pixel."""
    blocks = nonzero = 0
    for ti in range(len(X.TILES)):
        for n, lay, sel in X.layouts_of(fi, ti):
            if sel:  # (the selection of out / out8 does not enter the change)
                continue
            ch, seed = X.accumulate_shared_case(fi, ti, n, lay)
            owns = X.blocks_with_real_pixels(lay)
            for d in _expected_deltas(lay, ch, seed, 2, "none"):  # == the first two passes of "last"
                assert np.isfinite(d).all() and ((d != 0.0) == owns).all(), (lay.key(), d)
                blocks += len(d)
                nonzero += int(owns.sum())
    # (most blocks of a 64 x 64 tile on a small frame hold padding alone: the count is the frame's geometry)
    assert 0 < nonzero <= blocks, (blocks, nonzero)


def test_round_step_shared_layouts_reach_direct_with_empty_slots():
    """What test_round_step_shared_layouts runs: per frame and tile, the layouts whose rank has real pixels,
    and among them `direct` with -1 slots, world 3 with ranks 0 and 2, and pixels that stop in round 0 or 1."""
    for fi in range(len(X.FRAMES)):
        for ti in range(len(X.TILES)):
            with_px = stops = 0
            seen = set()
            for n, lay, sel in X.layouts_of(fi, ti):
                real, _ = X.out_index(lay)
                if not real.any():
                    continue
                with_px += 1
                holes = lay.order is not None and (lay.order[lay.rank::lay.world][:lay.slots] < 0).any()
                seen.add((lay.world, lay.rank, lay.direct, bool(holes)))
                st = X.pool_streams(min(int(real.sum()), 40), 7 * n + fi + 3 * ti, short=n % 2 == 1)
                stops += int((st.fold()["batches"] <= 2).sum())
            assert with_px >= 18 and stops > 0, (fi, ti, with_px, stops)
            assert (1, 0, 1, True) in seen
            if lay.n_tiles >= 6:  # (a frame of one or two tiles leaves a rank of three no slot to be empty)
                assert {(3, 0, 1, True), (3, 2, 1, True), (3, 2, 0, False)} <= seen, (fi, ti, sorted(seen))
    # a quarter at least stops in round 0, goes on from round 1 (long), stops in round 1 (short)
    long, short = X.pool_streams(64, 0).fold()["batches"], X.pool_streams(64, 0, short=True).fold()["batches"]
    assert (long == 1).mean() >= 0.25 and (long > 2).mean() >= 0.25 and (short == 2).mean() >= 0.25 and (short <= 2).all()


def test_color_byte_is_the_oracles():
    v = np.r_[np.linspace(-0.5, 1.5, 4001), [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-320, 0.998001, 0.999 ** 2, 1e300],
              (np.arange(257) / 256.0) ** 2]
    assert list(X.color_byte(v)) == [oracle.color_byte(float(x)) for x in v]


def test_udiv_make_is_exact():
    rng = np.random.default_rng(1)
    for d in (1, 2, 3, 5, 16, 17, 257, 65536, 0x7FFFFFFF, 0xFFFFFFFF):
        dd, m, s1, s2 = X.udiv_make(d)
        for n in [0, 1, d - 1, d, d + 1, 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 1 << 32, 200)]:
            n &= X.U32
            t = (n * m) >> 32
            assert (t + ((n - t) >> s1)) >> s2 == n // d


def test_tree_is_not_a_straight_sum():
    rng = np.random.default_rng(3)
    v = (10.0 ** rng.uniform(-8, 4, (64, 256)))
    tree = X.tree256(v)
    straight = np.zeros(64)
    for t in range(256):
        straight = straight + v[:, t]
    assert (X.bits(tree) != X.bits(straight)).mean() > 0.25
    # h = 128 first: thread 0 ends as ((v0 + v128) + (v64 + v192)) + ...
    w = np.zeros((1, 256))
    w[0, [0, 64, 128, 192]] = (1e16, 1.0, -1e16, 1.0)
    assert X.tree256(w)[0] == 2.0  # (1e16 + -1e16) + (1 + 1); a tree started at 64 would lose the ones


def test_within_wave_rule():
    src = np.arange(1000, 1200)
    assert X.within_wave_rule(src, np.r_[src[64:128:3], src[0:64:2], src[128:200]])
    assert not X.within_wave_rule(src, np.r_[src[2], src[0], src[4]])          # order inside a wave not kept
    assert not X.within_wave_rule(src, np.r_[src[0], src[70], src[2]])         # a wave's survivors split
    assert not X.within_wave_rule(src, np.r_[src[0], 7])                       # not an entry of the list
    assert X.within_wave_rule(src, np.zeros(0, dtype=np.int64))


# ------------------------------------------------------------------ the conditions on the cases
def test_fine_association_shows_in_the_bits():
    shown = shown32 = total = 0
    for fine_px_slots in (0, 2):
        for bs, chunk in ((10, 4), (16, 16)):
            ch = X.Chunking(64 * 8, bs, 2, chunk, fine_px_slots * 64)
            part = X.make_partial(ch, bs + fine_px_slots, specials=False)
            acc = np.zeros((ch.cap, 3))
            a = X.add_chunks(ch, part, acc)[ch.fine_px:]
            b = X.add_fine_straight(ch, part, acc)
            if chunk < bs:
                shown += int((X.bits(a) != X.bits(b)).any(axis=1).sum())
                # gs_combine_kernel shows only f32 colours: the cancelling pixels carry the difference there
                shown32 += int((X.bits(X.to_f32(a / float(bs))) != X.bits(X.to_f32(b / float(bs)))).any(axis=1).sum())
                total += len(a)
            else:  # one chunk: ((0 + s0) + s1) + ... then 0 + that: the same sums
                assert X.same_bits(a, b)
    assert total > 0 and shown / total >= 0.25 and shown32 / total >= 0.25, (shown, shown32, total)


def test_threshold_cases_fall_on_both_sides():
    cases = X.threshold_cases()
    assert len(cases) == 3 * 3 * 8
    first = np.array([st.fold()["batches"][0] == 1 for st in cases])
    share = first.mean()
    assert 0.25 <= share <= 0.75, share
    for move in (-1, 0, 1):  # and the ulp moves matter: every move has launches on its own
        assert any(("_m%d_" % move) in st.name for st in cases)
    # at the threshold itself, the pixel's test is within a few ulps of equality
    st = cases[8]
    s = st.fold()["sums"][0, 0]
    n = float(st.bs)
    conv = X.CONF * X.CONF * (1.0 / (n - 1.0) * (s[4] - s[3] * s[3] / n)) / n
    rhs = (s[3] / n) * (s[3] / n) * (st.tol * st.tol)
    assert abs(conv - rhs) <= 8 * np.spacing(conv)


def test_constant_cases_fall_on_both_sides():
    st = X.constant_case()
    f = st.fold()
    first = (f["batches"] == 1).mean()
    assert 0.25 <= first <= 0.75, first
    assert (f["reason"][f["batches"] < st.nb] == oracle.FOLD_CONVERGED).all()


def test_every_stop_reason_and_family_property():
    fams = {st.name: st for st in X.family_cases() if not st.name.startswith("thr_")}
    black = fams["black"].fold()
    assert (black["reason"] == oracle.FOLD_MAX_SAMPLES).all() and (black["batches"] == fams["black"].nb).all()
    k, bs = 2, 4
    assert (fams["max_kbs_minus_1"].fold()["batches"] <= k).all() and (fams["max_kbs_minus_1"].fold()["batches"] == k).any()
    assert (fams["max_kbs"].fold()["batches"] == k + 1).any() and (fams["max_kbs"].fold()["batches"] <= k + 1).all()
    assert (fams["max_zero"].fold()["batches"] == 1).all()
    assert (fams["max_u32max"].fold()["reason"] == oracle.FOLD_EXHAUSTED).any()
    ni = fams["nan_inf"]
    f = ni.fold()
    bad = ~np.isfinite(ni.samples).all(axis=(1, 2))
    at = np.argmax(~np.isfinite(ni.samples).all(axis=2), axis=1) // ni.bs  # the batch of the bad sample
    met = bad & (f["batches"] > at)  # (a pixel may converge before it comes)
    assert met.sum() >= 20 and (f["reason"][met] == oracle.FOLD_MAX_SAMPLES).all()  # NaN sums: no test is true
    assert (at[met] == 0).any() and (at[met] > 0).any()
    assert (~np.isfinite(f["color"][met])).any(axis=1).all() and (f["reason"][~bad] == oracle.FOLD_CONVERGED).any()
    neg = fams["negative"].fold()
    assert (fams["negative"].samples <= 0).all() and (neg["reason"] == oracle.FOLD_CONVERGED).sum() > 20
    assert (neg["color"] < 0).all()
    b1 = fams["bs1"].fold()
    assert (b1["batches"] >= 2).all() and (b1["batches"][::2] == 2).all()  # the first test is NaN; constants stop at the second
    mixed = X.mixed_case(1000, 4, 12, 4242).fold()
    assert set(mixed["reason"].tolist()) == {oracle.FOLD_CONVERGED, oracle.FOLD_MAX_SAMPLES}
    assert len(set(mixed["batches"].tolist())) == 12  # some pixel ends in every round of the chain
    for bs in (1, 2, 3, 16, 257):  # the shapes' cases keep enough pixels active in round 1
        for seg_n in (1, 63, 64, 65, 1000):
            n = seg_n + 40 + (600 if seg_n == 1000 else 200)
            st = X.mixed_case(n, bs, 3, 100 * seg_n + bs)
            a0, _ = X.round_inputs(st, 0)
            a1, _ = X.round_inputs(st, 1)
            assert len(a0) == n and len(a1) - 7 >= (seg_n if seg_n < 1000 else 501), (bs, seg_n, len(a1))
            stops0 = X.round_expect(st, 0, a0)[0]
            assert 0 < stops0.sum() < n or bs == 1


def test_params_table_takes_every_branch_and_matches_hand_values():
    seen = set()
    for name, a in X.params_table():
        f, hint, branch = X.round_params_ref(**a)
        seen.add(branch)
        assert f["n_items"] == (f["seg_n"] * f["cpp"]) & X.U32 and f["claim"] >= 1
    want = {"requested", "long_paths"} | {"halved_to_%d" % c for c in (16, 8, 4, 2, 1)}
    assert want <= seen and any(b.startswith("whole/halved") for b in seen), sorted(seen)
    # by hand: 5000 pixels of 16 samples over 1024 lanes, short paths: 16-sample items give 5000 < 8192 items,
    # 8-sample items 10000 >= 8192: csz 8, cpp 2, 10000 items; claim = min(32, 10000 / 16 waves / 4 = 156) = 32
    f, hint, _ = X.round_params_ref(1, 0, 1 << 20, 0, 0, 16, 1024, 16, 1 << 16, 5000, (100, 100), (0, 0))
    assert (f["chunk"], f["cpp"], f["n_items"], f["claim"], f["per_sample"]) == (8, 2, 10000, 32, 1)
    assert (f["u_d"], f["u_m"], f["u_s1"], f["u_s2"]) == (2, 1, 1, 0) and hint == (100, 100)
    assert (f["active"], f["next_active"], f["round_base"], f["fine_px"], f["fine_base"]) == (1, 0, 16, 1 << 16, X.U32)
    # 2 rays a path: 1-sample items whatever the count; claim's cap is GS_CLAIM_FINE: 80000 / 16 / 4 = 1250 -> 128
    f, hint, _ = X.round_params_ref(2, 0, 1 << 20, 0, 0, 16, 1024, 16, 1 << 16, 5000, (200, 100), (0, 0))
    assert (f["chunk"], f["cpp"], f["n_items"], f["claim"]) == (1, 16, 80000, 128) and hint == (200, 100)
    # segment 2 of 1000 pixels when 2500 are active: base 2000, 500 left; whole-batch items on request
    f, _, _ = X.round_params_ref(0, 2, 1000, 0, 1, 256, 64, 4, 4096, 2500, None, (0, 0))
    assert (f["seg_base"], f["seg_n"], f["per_sample"], f["chunk"], f["cpp"], f["n_items"]) == (2000, 500, 0, 0, 1, 500)
    assert f["claim"] == min(32, 500 // 4 // 4)
    # ... but not for a batch of 257, nor with a requested chunk (40 > bs 16 -> 16)
    assert X.round_params_ref(0, 0, 1000, 0, 1, 257, 64, 4, 4096, 2500, None, (0, 0))[0]["per_sample"] == 1
    f, _, _ = X.round_params_ref(0, 0, 1000, 40, 1, 16, 64, 4, 4096, 2500, None, (0, 0))
    assert (f["per_sample"], f["chunk"], f["cpp"]) == (1, 16, 1)
    # whole_mode -1: whole at n_seg = 2 lanes, split one below
    assert X.round_params_ref(1, 0, 1 << 20, 0, -1, 16, 1024, 16, 1 << 16, 2048, None, (0, 0))[0]["per_sample"] == 0
    assert X.round_params_ref(1, 0, 1 << 20, 0, -1, 16, 1024, 16, 1 << 16, 2047, None, (0, 0))[0]["per_sample"] == 1


def test_view_cases_have_both_selection_states():
    lay = X.Layout(24, 48, 8, 8, 1, 0, None, 0, slots=19)
    for selected, before in (((1, 0, 1), (0, 8, 0)), ((0, 1, 1), (16, 0, 8))):
        vs = np.array(list(zip(before, selected)), dtype=np.uint32)
        order = X.views_order_ref(lay, None, vs, 16)
        assert (order[:18].reshape(3, 6) >= 0).all(axis=1).tolist() == [bool(s) for s in selected] and order[18] == -1
        ch = X.Chunking(lay.cap, 8, 2, 4, lay.cap)
        acc0 = np.random.default_rng(1).uniform(1, 2, (lay.cap, 3))
        ea, eo, _, ev = X.views_accumulate_ref(lay, ch, None, vs, 16, X.make_partial(ch, 1, specials=False), acc0)
        view = np.arange(lay.cap) // (6 * 64)
        for v in range(3):
            m = view == v
            assert (X.bits(ea[m]) == X.bits(acc0[m])).all() == (not selected[v])
            assert (ev[6 * v:6 * v + 6] != 0).all() == bool(selected[v])
            if not selected[v] and before[v] == 0:
                assert (X.bits(eo[m]) == 0).all()  # resolves to +0.0, not 0 / 0
            if not selected[v] and before[v]:
                assert X.same_bits(eo[m], X.to_f32(acc0[m] / float(before[v])))
        assert (eo[view == 3] == 0).all() and ev[18] == 0.0


def test_resolve_reference_edges():
    lay = X.layout(21, 13, 8, 8)
    real, _ = X.out_index(lay)
    ps = np.zeros((lay.cap, 5))
    word = np.zeros(lay.cap, dtype=np.uint32)
    k = np.flatnonzero(real)[:4]
    ps[k[0]] = (8.0, 16.0, 24.0, 0.0, 1.0)          # mean 0: the error is x / 0 = inf
    ps[k[1]] = (8.0, 16.0, 24.0, 8.0, 1.0)          # lsq < lsum^2 / n: sqrt of a negative = NaN
    ps[k[2]] = (8.0, 16.0, 24.0, 8.0, 9.0)
    word[k[0]], word[k[1]], word[k[2]], word[k[3]] = 2, 2 | X.STOPPED, 0x7FFFFFFF, 1
    out, out8, ms, me, summary = X.resolve_ref(lay, 4, 2.0, ps, word)
    assert tuple(out[k[0]]) == (1.0, 2.0, 3.0) and np.isinf(me[k[0]]) and np.isnan(me[k[1]])
    assert ms[k[0]] == 8 and ms[k[2]] == X.U32 and ms[k[3]] == 4
    n_real = int(real.sum())
    assert summary == (n_real - 1, 8 + 8 + 4 * 0x7FFFFFFF + 4, 4 * 0x7FFFFFFF)
    _, _, _, me1, _ = X.resolve_ref(lay, 1, 2.0, ps, np.where(real, 1, 0).astype(np.uint32))
    assert np.isnan(me1[k[2]])  # one round of a one-sample batch: 1 / 0 * (9 - 64) = -inf, and its sqrt is NaN
    ps[k[2], 4] = 64.0           # ... and a true single sample has lsq = lsum^2: inf * 0 = NaN
    assert np.isnan(X.resolve_ref(lay, 1, 2.0, ps, np.where(real, 1, 0).astype(np.uint32))[3][k[2]])
