"""Cases and reference for the known-answer tests of the pixel stage (grayshift_amd/csrc/device/pixel.hpp):
the kernels that turn samples into pixels.

Two references.  What is camera.rs -- a batch folded into the running sums in sample order and the stop
test (camera.rs:135-167) -- is the oracle's own loop, oracle.sample_fold.  What is layout and scheduling
is restated here in plain numpy f64, elementwise and in the kernels' order: packed_pixel, the coarse and
fine indexing of `partial`, the re-forming of 1-sample sums into chunks, the thread-strided-then-tree
reduction of delta / vdelta, the resolve's maps and the item-size rule of gs_round_params_kernel.  numpy's
+ - * / sqrt and casts are IEEE and never contract, so the results are bit-exact.

tests/test_pixel_cases_host.py asserts on these references alone that the cases reach the edges;
tests/test_gpu_pixel_kat.py runs the kernels on them."""
import numpy as np

STOPPED = 0x80000000           # GS_ADAPT_STOPPED
ACCUM_MAX_BLOCKS = 2048        # GS_ACCUM_MAX_BLOCKS
CLAIM_DIV, CLAIM_FINE, WHOLE_MAX_BATCH = 4, 128, 256  # GS_CLAIM_DIV, GS_CLAIM_FINE, GS_ROUND_WHOLE_MAX_BATCH
U32 = 0xFFFFFFFF
F32_POISON = np.float32(-7.5)  # what an untouched f32 output holds
U8_POISON = 0xA5
NAN_POISON = np.float64("nan")

FRAMES = ((1, 1), (21, 13), (80, 45))
TILES = ((8, 8), (16, 4), (64, 64))
RANKS = ((1, 0), (3, 0), (3, 2))
ORDERS = ("none", "perm", "holes")


def accum_blocks(cap):
    return 1 if cap == 0 else min((cap - 1) // 256 + 1, ACCUM_MAX_BLOCKS)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN at the same place whatever its payload."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (bits(a)[~na] == bits(b)[~na]).all())


def where_differs(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return np.argwhere(a != b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.argwhere((na != nb) | (~na & ~nb & (bits(a) != bits(b))))


# ------------------------------------------------------------------ the layout: packed_pixel
class Layout:
    """A frame, its tiles, one rank's slots and the tile order (None, or int32 [n_pos] with -1 for an
    empty slot)."""

    def __init__(self, W, H, tw, th, world=1, rank=0, order=None, direct=0, slots=None):
        self.W, self.H, self.tw, self.th, self.world, self.rank, self.direct = W, H, tw, th, world, rank, direct
        self.tiles_x, self.tiles_y = -(-W // tw), -(-H // th)
        self.n_tiles = self.tiles_x * self.tiles_y
        self.order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        if slots is None:
            n_pos = self.n_tiles if order is None else len(self.order)
            slots = max(1, -(-n_pos // world))
        self.slots = slots
        self.n_pos = slots * world if order is None else len(self.order)
        self.tile_px = tw * th
        self.cap = slots * self.tile_px
        self.n_out = W * H if direct else self.cap

    def key(self):
        return "%dx%d_t%dx%d_w%dr%d_d%d" % (self.W, self.H, self.tw, self.th, self.world, self.rank, self.direct)


def make_order(W, H, tw, th, world, kind, seed):
    """None; a permutation of the tiles over the positions (positions past the tiles are -1, as a plan
    leaves them); or a permutation with further -1 slots strewn in."""
    if kind == "none":
        return None
    n_tiles = (-(-W // tw)) * (-(-H // th))
    rng = np.random.default_rng(seed)
    holes = 0 if kind == "perm" else 1 + n_tiles // 3
    n_pos = -(-(n_tiles + holes) // world) * world
    order = np.full(n_pos, -1, dtype=np.int32)
    order[rng.permutation(n_pos)[:n_tiles]] = rng.permutation(n_tiles).astype(np.int32)
    if kind == "perm" and n_pos == n_tiles:
        assert sorted(order) == list(range(n_tiles))
    return order


def layout(W, H, tw, th, world=1, rank=0, kind="none", direct=0, seed=1):
    order = make_order(W, H, tw, th, world, kind, seed)
    if order is None:  # one slot more than the tiles need: positions past the last tile are padding
        n_tiles = (-(-W // tw)) * (-(-H // th))
        return Layout(W, H, tw, th, world, rank, None, direct, slots=-(-n_tiles // world) + 1)
    return Layout(W, H, tw, th, world, rank, order, direct)


def layouts_of(fi, ti):
    """The shared layout cases of frame fi and tile ti: (n, layout, sel) over rank x order x direct x the
    selection of out / out8 (outsel).  The GPU tests and the host assertions both iterate this."""
    W, H = FRAMES[fi]
    tw, th = TILES[ti]
    n = 0
    for (world, rank) in RANKS:
        for oi, kind in enumerate(ORDERS):
            for direct in (0, 1):
                for sel in range(3):
                    yield n, layout(W, H, tw, th, world, rank, kind, direct, seed=100 * fi + 10 * ti + oi), sel
                    n += 1


def outsel(i):
    """out only, out8 only, both."""
    return ((True, False), (False, True), (True, True))[i % 3]


def shared_layouts():
    """The shared layout cases: every frame x tile x rank x order x direct."""
    return [lay for fi in range(len(FRAMES)) for ti in range(len(TILES)) for n, lay, sel in layouts_of(fi, ti) if sel == 0]


def packed_pixel(lay, order="own"):
    """packed_pixel for every packed slot k of the rank: (real [cap] bool, pi, pj int64)."""
    order = lay.order if isinstance(order, str) else order
    k = np.arange(lay.cap, dtype=np.int64)
    slot, w = k // lay.tile_px, k % lay.tile_px
    pos = lay.rank + slot * lay.world
    tile = pos if order is None else order[pos].astype(np.int64)
    empty = tile < 0
    t = np.where(empty, 0, tile)
    pi = (t % lay.tiles_x) * lay.tw + w % lay.tw
    pj = (t // lay.tiles_x) * lay.th + w // lay.tw
    real = ~empty & (pi < lay.W) & (pj < lay.H)
    return real, pi, pj


def out_index(lay, order="own"):
    """(real, the index of packed pixel k in out / out8)."""
    real, pi, pj = packed_pixel(lay, order)
    return real, (pj * lay.W + pi if lay.direct else np.arange(lay.cap, dtype=np.int64))


def color_byte(c):
    """write_color's byte (color.rs:8-28), elementwise: sqrt of a positive value else 0, clamp to
    [0, 0.999], (256 c) truncated."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        g = np.where(c > 0.0, np.sqrt(np.where(c > 0.0, c, 0.0)), 0.0)
        g = np.where(g > 0.999, 0.999, g)
        return (256.0 * g).astype(np.int32).astype(np.uint8)


def to_f32(c):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(c, dtype=np.float64).astype(np.float32)


def poison_outputs(lay, want_out=True, want_out8=True):
    out = np.full((lay.n_out, 3), F32_POISON, dtype=np.float32) if want_out else None
    out8 = np.full((lay.n_out, 3), U8_POISON, dtype=np.uint8) if want_out8 else None
    return out, out8


def expected_outputs(lay, colour, written, order="own", want_out=True, want_out8=True):
    """out / out8 after a kernel that resolves `colour` [cap,3] for the real pixels in `written` [cap]:
    packed mode zeroes the padding slots, `direct` leaves padding and unowned pixels alone."""
    real, oi = out_index(lay, order)
    out, out8 = poison_outputs(lay, want_out, want_out8)
    w = real & written
    if out is not None:
        if not lay.direct:
            out[~real] = 0.0
        out[oi[w]] = to_f32(colour[w])
    if out8 is not None:
        if not lay.direct:
            out8[~real] = 0
        out8[oi[w]] = color_byte(colour[w])
    return out, out8


# ------------------------------------------------------------------ chunk sums: coarse, fine, re-formed
class Chunking:
    """`partial`'s layout for a launch: coarse pixels [0, fine_px) hold cpp chunk sums each, chunk ck of
    pixel k at ck * fine_px + k; fine pixels [fine_px, cap) hold bs 1-sample sums each from fine_base on,
    sample s of pixel k at fine_base + s * (cap - fine_px) + k - fine_px."""

    def __init__(self, cap, bs, cpp, chunk, fine_px):
        self.cap, self.bs, self.cpp, self.chunk, self.fine_px = cap, bs, cpp, chunk, fine_px
        self.fine_base = fine_px * cpp
        self.n = max(1, self.fine_base + bs * (cap - fine_px)) * 3


def add_chunks(ch, partial, acc):
    """acc [cap,3] + the launch's sums in the kernels' order: ((acc + C_0) + C_1) + ...; a fine pixel's
    1-sample sums first re-formed into chunks of ch.chunk, each from 0.0."""
    p3 = partial.reshape(-1, 3)
    r = acc.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.arange(ch.fine_px)
        for c in range(ch.cpp if ch.fine_px else 0):
            r[k] = r[k] + p3[c * ch.fine_px + k]
        nf = ch.cap - ch.fine_px
        kk = np.arange(nf)
        if nf:
            for s0 in range(0, ch.bs, ch.chunk):
                cs = np.zeros((nf, 3))
                for s in range(s0, min(ch.bs, s0 + ch.chunk)):
                    cs = cs + p3[ch.fine_base + s * nf + kk]
                r[ch.fine_px + kk] = r[ch.fine_px + kk] + cs
    return r


def add_fine_straight(ch, partial, acc):
    """The fine pixels' sums added straight through, sample after sample (what the kernels must NOT do)."""
    p3 = partial.reshape(-1, 3)
    nf = ch.cap - ch.fine_px
    kk = np.arange(nf)
    r = acc[ch.fine_px:].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(ch.bs):
            r = r + p3[ch.fine_base + s * nf + kk]
    return r


SPECIALS = (0.0, -0.0, 5e-324, -2.5e-310, 3.5e38, -1e39, 1e300, np.inf, -np.inf, np.nan)


def make_partial(ch, seed, specials=True):
    """Sums whose magnitudes run from 1e-12 to 1e6 with both signs, so that the association of the
    additions shows in the bits; `specials` strews +-0, denormals, values past f32's range, inf and NaN."""
    rng = np.random.default_rng(seed)
    p = (10.0 ** rng.uniform(-12.0, 6.0, ch.n)) * rng.choice([-1.0, 1.0], ch.n)
    nf = ch.cap - ch.fine_px
    if nf and ch.bs >= 2:
        # Every other fine pixel cancels: B and -B (1e3 .. 1e6) at two of its samples, the rest below 1e-6, so
        # what is left is the small samples' sum as the additions' order rounded it -- an association that is
        # off shows in the f32 colour too, not only in the f64 sums.
        fine = p[ch.fine_base * 3:(ch.fine_base + ch.bs * nf) * 3].reshape(ch.bs, nf, 3)
        k = np.arange(0, nf, 2)
        fine[:, k] *= 1e-12
        a = rng.integers(0, ch.bs, len(k))
        b = (a + 1 + rng.integers(0, ch.bs - 1, len(k))) % ch.bs
        big = 10.0 ** rng.uniform(3.0, 6.0, (len(k), 3))
        fine[a, k] = big
        fine[b, k] = -big
    if specials:
        m = min(ch.n, max(len(SPECIALS), ch.n // 50))
        p[rng.choice(ch.n, m, replace=False)] = rng.choice(np.array(SPECIALS), m)
    return p


def combine_ref(lay, ch, partial, want_out=True, want_out8=True):
    real, _ = out_index(lay)
    with np.errstate(invalid="ignore", over="ignore"):
        colour = add_chunks(ch, partial, np.zeros((lay.cap, 3))) / (0.0 + float(ch.bs))
    return expected_outputs(lay, colour, np.ones(lay.cap, dtype=bool), want_out=want_out, want_out8=want_out8)


# ------------------------------------------------------------------ the change's reduction
def tree256(v):
    """[blocks, 256] per-thread values folded as the kernels' LDS tree: h = 128, 64, ..., 1."""
    v = v.copy()
    h = 128
    with np.errstate(invalid="ignore", over="ignore"):
        while h > 0:
            v[:, :h] = v[:, :h] + v[:, h:2 * h]
            h >>= 1
    return v[:, 0].copy()


def strided_change(terms, blocks):
    """terms [cap,3]: a pixel's three |after - before| (0 where it adds none).  Thread g of blocks * 256
    takes pixels g, g + T, ... in order, three additions each; then the tree per block."""
    T = blocks * 256
    cap = len(terms)
    change = np.zeros(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, cap, T):
            t = terms[k0:k0 + T]
            for c in range(3):
                change[:len(t)] = change[:len(t)] + t[:, c]
    return tree256(change.reshape(blocks, 256))


def accumulate_ref(lay, ch, partial, acc, base, want_out=True, want_out8=True):
    """One pass of gs_accumulate_kernel: (accum after, out, out8, delta [gs_accum_blocks])."""
    real, _ = out_index(lay)
    r = add_chunks(ch, partial, acc)
    r = np.where(real[:, None], r, acc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        colour = r / float(base + ch.bs)
        before = acc / float(base) if base else np.zeros_like(acc)
        terms = np.where(real[:, None], np.abs(colour - before), 0.0)
    out, out8 = expected_outputs(lay, colour, np.ones(lay.cap, dtype=bool), want_out=want_out, want_out8=want_out8)
    return r, out, out8, strided_change(terms, accum_blocks(lay.cap))


def chunkings(cap, tile_px):
    """cpp in {1, 2, 5} x fine_px in {0, a tile multiple inside, capacity} x the fine path's (bs 10, chunk 4:
    chunks of 4, 4, 2) and (bs 16, chunk 16)."""
    slots = cap // tile_px
    inside = (slots // 2) * tile_px if slots > 1 else 0
    out = []
    for cpp in (1, 2, 5):
        for fine_px in (0, inside, cap):
            for bs, chunk in ((10, 4), (16, 16)):
                out.append(Chunking(cap, bs, cpp, chunk, fine_px))
    return out


def accumulate_parts(ch, seed, n_pass, specials):
    """The sums of n_pass chained passes [n_pass, ch.n].  specials: "none"; "all" (every pass: a NaN or an inf
    then lives on in accum, and in every later change of its block); "last" (the last pass alone: the change
    of every earlier pass is finite, so those are compared as numbers)."""
    assert specials in ("none", "all", "last")
    return np.stack([make_partial(ch, seed + p, specials=(specials == "all" or (specials == "last" and p == n_pass - 1)))
                     for p in range(n_pass)])


ACC_LAYOUTS = {"cap64": lambda d: Layout(7, 5, 8, 8, 1, 0, None, d, slots=1),          # a partial block
               "cap256": lambda d: Layout(30, 6, 16, 4, 1, 0, None, d, slots=4),       # exactly one
               "cap320": lambda d: Layout(37, 8, 8, 8, 1, 0, None, d, slots=5),        # one and a quarter
               "cap528384": lambda d: Layout(43 * 64 - 10, 3 * 64 - 5, 64, 64, 1, 0, None, d, slots=129)}


def accumulate_named_cases(name):
    """The runs of three chained passes at a named capacity: (layout, chunking, seed, specials, with_delta).
    The small capacities run clean sums (every block's change a finite number in every pass) and sums with
    specials in every pass, both with `direct` 0 and 1, and once with delta null."""
    big = name == "cap528384"
    out = []
    for direct in ((0,) if big else (0, 1)):
        lay = ACC_LAYOUTS[name](direct)
        assert lay.cap == int(name[3:])
        inside = 128 * lay.tile_px if big else (lay.slots // 2) * lay.tile_px
        ch = Chunking(lay.cap, 8, 2, 4, inside)
        out.append((lay, ch, 31 + direct, "none", True))
        if not big:
            out.append((lay, ch, 41 + direct, "all", True))
    if not big:
        out.append((lay, Chunking(lay.cap, 10, 3, 4, 0), 77, "all", False))
    return out


def accumulate_shared_case(fi, ti, n, lay):
    """test_accumulate_shared_layouts' run on a shared layout: (chunking, seed); three passes, specials in
    the last."""
    chs = chunkings(lay.cap, lay.tile_px)
    return chs[(5 * n + fi + ti) % len(chs)], 2000 * fi + 200 * ti + n


def blocks_with_real_pixels(lay):
    """[gs_accum_blocks] bool: does the block's grid-stride share of the packed pixels hold a real one?"""
    blocks = accum_blocks(lay.cap)
    real, _ = out_index(lay)
    T = blocks * 256
    r = np.zeros(-(-lay.cap // T) * T, dtype=bool)
    r[:lay.cap] = real
    return r.reshape(-1, blocks, 256).any(axis=(0, 2))


# ------------------------------------------------------------------ views
def views_order_ref(lay, vorder, vstate, view_h):
    """gs_views_order_kernel: position -> its tile, or -1 (an empty position, a tile outside the frame or
    of an unselected view)."""
    pos = np.arange(lay.n_pos, dtype=np.int64)
    tile = pos if vorder is None else vorder.astype(np.int64)
    row = (np.where(tile < 0, 0, tile) // lay.tiles_x) * lay.th
    ok = (tile >= 0) & (row < lay.H)
    sel = np.zeros(lay.n_pos, dtype=bool)
    sel[ok] = vstate[row[ok] // view_h, 1] != 0
    return np.where(ok & sel, tile, -1).astype(np.int32)


def views_accumulate_ref(lay, ch, vorder, vstate, view_h, partial, acc, want_out=True, want_out8=True):
    """gs_views_accumulate_kernel: (accum after, out, out8, vdelta [slots])."""
    real, pi, pj = packed_pixel(lay, vorder)
    view = np.where(real, pj // view_h, 0)
    before = vstate[view, 0].astype(np.int64)
    sel = real & (vstate[view, 1] != 0)
    n_after = np.where(sel, before + ch.bs, before)
    summed = add_chunks(ch, partial, acc)
    r = np.where(sel[:, None], summed, acc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        colour = np.where((n_after > 0)[:, None], r / np.maximum(n_after, 1).astype(np.float64)[:, None], 0.0)
        prev = np.where((before > 0)[:, None], acc / np.maximum(before, 1).astype(np.float64)[:, None], 0.0)
        terms = np.where(sel[:, None], np.abs(colour - prev), 0.0)
    colour = np.where(real[:, None], colour, 0.0)
    out, out8 = expected_outputs(lay, colour, np.ones(lay.cap, dtype=bool), order=vorder, want_out=want_out,
                                 want_out8=want_out8)
    # one block per slot: thread t takes the slot's pixels t, t + 256, ...
    tpx = lay.tile_px
    per = np.zeros((lay.slots, 256))
    with np.errstate(invalid="ignore", over="ignore"):
        for w0 in range(0, tpx, 256):
            n = min(256, tpx - w0)
            idx = (np.arange(lay.slots) * tpx)[:, None] + w0 + np.arange(n)[None, :]
            for c in range(3):
                per[:, :n] = per[:, :n] + terms[idx, c]
    vdelta = tree256(per)
    return r, out, out8, vdelta


# ------------------------------------------------------------------ gs_round_params_kernel
def udiv_make(d):
    l = 0
    while l < 32 and (1 << l) < d:
        l += 1
    return (d, (((1 << 32) * ((1 << l) - d)) // d + 1) & U32, min(l, 1), 0 if l < 1 else l - 1)


PARAMS_FIELDS = ("per_sample", "chunk", "round", "cpp", "u_d", "u_m", "u_s1", "u_s2", "n_items", "fine_base",
                 "fine_px", "claim", "claim_fine", "round_base", "seg_base", "seg_n", "active", "next_active", "queue")


def round_params_ref(round, seg, seg_px, chunk_req, whole_mode, bs, lanes, waves, capacity, n_act, counters, hint):
    """Every field gs_round_params_kernel writes, the hint after it, and the branch taken.  counters:
    (rays, paths) or None; hint: (rays, paths)."""
    base = (seg * seg_px) & U32
    n_seg = min(seg_px, n_act - base) if n_act > base else 0
    whole = chunk_req <= 0 and bs <= WHOLE_MAX_BATCH and (whole_mode > 0 or (whole_mode < 0 and n_seg >= 2 * lanes))
    hint = tuple(hint)
    if chunk_req > 0:
        csz, branch = min(chunk_req, bs), "requested"
    else:
        rays = paths = 0
        if round and counters is not None:
            rays, paths = counters
            hint = (rays, paths)
        elif not round:
            rays, paths = hint
        if paths and rays >= 2 * paths:
            csz, branch = 1, "long_paths"
        else:
            csz = min(16, bs)
            while csz > 1 and n_seg * ((bs + csz - 1) // csz) < 8 * lanes:
                csz >>= 1
            branch = "halved_to_%d" % csz
    if whole:
        branch = "whole/" + branch
    cpp = 1 if whole else (bs + csz - 1) // csz
    n_items = (n_seg * cpp) & U32
    claim = max(1, min(32 if (whole or csz > 4) else CLAIM_FINE, n_items // max(1, waves) // CLAIM_DIV))
    u = udiv_make(cpp)
    f = {"per_sample": 0 if whole else 1, "chunk": 0 if whole else csz, "round": round, "cpp": cpp, "u_d": u[0],
         "u_m": u[1], "u_s1": u[2], "u_s2": u[3], "n_items": n_items, "fine_base": U32, "fine_px": capacity,
         "claim": claim, "claim_fine": claim, "round_base": (round * bs) & U32, "seg_base": base, "seg_n": n_seg,
         "active": round & 1, "next_active": (round & 1) ^ 1, "queue": 0}
    return f, hint, branch


def params_table():
    """(name, arguments of round_params_ref) over the item-size rule's branches."""
    T = []

    def add(name, round=1, seg=0, seg_px=1 << 20, chunk_req=0, whole_mode=0, bs=16, lanes=1024, waves=16,
            capacity=1 << 16, n_act=5000, counters=(100, 100), hint=(0, 0)):
        T.append((name, dict(round=round, seg=seg, seg_px=seg_px, chunk_req=chunk_req, whole_mode=whole_mode, bs=bs,
                             lanes=lanes, waves=waves, capacity=capacity, n_act=n_act, counters=counters, hint=hint)))

    for n_act in (2999, 3000, 3001, 2000, 1999, 999, 1000, 1001):  # seg 2 of 1000: below, at, above seg * seg_px
        add("seg2_nact%d" % n_act, seg=2, seg_px=1000, n_act=n_act)
    for cr in (0, 3, 40):
        for bs in (16, 7):
            add("chunk_req%d_bs%d" % (cr, bs), chunk_req=cr, bs=bs)
    for wm in (-1, 0, 1):
        for bs in (256, 257):
            for n_act in (2 * 1024 - 1, 2 * 1024):
                add("whole%d_bs%d_n%d" % (wm, bs, n_act), whole_mode=wm, bs=bs, n_act=n_act)
        add("whole%d_chunk_req" % wm, whole_mode=wm, chunk_req=4, n_act=4096)
    add("round0_hint_long", round=0, hint=(20, 10), counters=(1, 1))
    add("round0_hint_short", round=0, hint=(19, 10), counters=(50, 10))
    add("round0_hint_empty", round=0, hint=(0, 0), counters=None)
    add("round3_counters_long", round=3, counters=(2 * 777, 777), hint=(5, 5))
    add("round3_counters_short", round=3, counters=(2 * 777 - 1, 777), hint=(50, 5))
    add("round3_no_counters", round=3, counters=None, hint=(50, 5))
    add("round2_no_paths", round=2, counters=(9, 0), hint=(50, 5))
    # the halving loop: n_seg * ceil(bs / csz) < 8 lanes halves; ends at 16, 8, ..., 1
    for n_act, lanes in ((8192, 1024), (8191, 1024), (4096, 1024), (4095, 1024), (2048, 1024), (1024, 1024), (1023, 1024),
                         (512, 1024), (511, 1024), (1, 1024), (0, 1024), (100, 0)):
        add("halve_n%d_l%d" % (n_act, lanes), n_act=n_act, lanes=lanes)
    add("halve_bs5", bs=5, n_act=3000)
    add("halve_bs1", bs=1, n_act=10)
    # claim: floor 1, the caps 32 (items of more than 4 samples, whole) and GS_CLAIM_FINE, waves 0
    add("claim_floor", n_act=3, waves=64)
    add("claim_cap32", n_act=1 << 20, waves=4, capacity=1 << 21)
    add("claim_cap32_at", n_act=32 * 4 * 4, waves=4, lanes=1)
    add("claim_cap32_below", n_act=32 * 4 * 4 - 1, waves=4, lanes=1)
    add("claim_cap_fine", n_act=1 << 16, waves=2, counters=(300, 100))
    add("claim_fine_at", n_act=CLAIM_FINE * 2 * CLAIM_DIV // 16, waves=2, counters=(300, 100))
    add("claim_fine_csz4", n_act=1 << 16, waves=2, chunk_req=4)
    add("claim_coarse_csz5", n_act=1 << 16, waves=2, chunk_req=5)
    add("claim_whole", n_act=1 << 16, waves=2, whole_mode=1)
    add("claim_waves0", n_act=1000, waves=0)
    return T


# ------------------------------------------------------------------ the rounds: streams and the fold
CONF = 1.96


def first_batch_tolerance(samples, bs, conf):
    """sqrt(convergence) / |mean| of a pixel's first batch, in the stop test's own operations."""
    import oracle
    s = oracle.sample_fold(samples[None, :bs], bs, conf, 0.0, U32)["sums"][0, 0]
    n = float(bs)
    mean = s[3] / n
    var = 1.0 / (n - 1.0) * (s[4] - s[3] * s[3] / n)
    conv = conf * conf * var / n
    return float(np.sqrt(conv) / abs(mean))


class Streams:
    """One launch's worth of pixels: samples [n, S, 3] and the launch's settings."""

    def __init__(self, name, samples, bs, tol, max_samples, conf=CONF):
        self.name, self.samples, self.bs, self.tol, self.max_samples, self.conf = name, samples, bs, tol, max_samples, conf
        self.n, self.S = samples.shape[0], samples.shape[1]
        self.nb = self.S // bs
        self._fold = None

    def fold(self):
        """oracle.sample_fold of every whole stream (computed once)."""
        if self._fold is None:
            import oracle
            self._fold = oracle.sample_fold(self.samples, self.bs, self.conf, self.tol, self.max_samples)
        return self._fold


def random_colours(rng, n, S, scale):
    """Colours around a per-pixel base: relative spread 2 % to 60 %, so some pixels converge in the first
    batches and others run on."""
    base = scale * rng.uniform(0.1, 1.0, (n, 1, 3))
    spread = rng.choice([0.02, 0.1, 0.3, 0.6], (n, 1, 1))
    return base * (1.0 + spread * rng.uniform(-1.0, 1.0, (n, S, 3)))


def threshold_cases(bs=8, nb=3, per=8, n=16):
    """Launches whose tolerance sits on pixel 0's first-batch threshold, one ulp below it, or one above:
    random colours at scales 1e-3, 1, 50.  The pixel of interest is pixel 0 of each launch."""
    out = []
    for si, scale in enumerate((1e-3, 1.0, 50.0)):
        for move in (-1, 0, 1):
            for j in range(per):
                rng = np.random.default_rng(7000 + 100 * si + 10 * (move + 1) + j)
                smp = random_colours(rng, n, nb * bs, scale)
                t = first_batch_tolerance(smp[0], bs, CONF)
                t = t if move == 0 else float(np.nextafter(t, np.inf if move > 0 else 0.0))
                out.append(Streams("thr_s%d_m%d_%d" % (si, move, j), smp, bs, t, nb * bs - 1))
    return out


def constant_case(n=600, bs=8, nb=3, seed=11):
    """Constant-colour pixels at tolerance 0: `convergence < 0` holds only where the rounding residue of
    lsq - lsum * lsum / scount is negative."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.01, 2.0, (n, 1, 3)) * (10.0 ** rng.integers(-3, 3, (n, 1, 1)))
    return Streams("constant_tol0", np.repeat(c, nb * bs, axis=1), bs, 0.0, nb * bs - 1)


def black_case(n=100, bs=4, nb=3):
    return Streams("black", np.zeros((n, nb * bs, 3)), bs, 1e30, nb * bs - 1)


def max_samples_cases(n=200, bs=4, nb=4, k=2, seed=13):
    """Noisy pixels under a tight tolerance, so max_samples ends them: k bs - 1 (stops after batch k), k bs
    (after k + 1), 0 (after the first), 2^32 - 1 (never)."""
    rng = np.random.default_rng(seed)
    smp = random_colours(rng, n, nb * bs, 1.0)
    return [Streams("max_%s" % nm, smp, bs, 1e-9, m)
            for nm, m in (("kbs_minus_1", k * bs - 1), ("kbs", k * bs), ("zero", 0), ("u32max", U32))]


def nan_inf_case(n=120, bs=4, nb=3, seed=17):
    """A NaN sample (sums NaN: no test ever true but max_samples') and an inf sample (inf - inf in the
    variance), in the first, a middle or the last batch, next to clean pixels."""
    rng = np.random.default_rng(seed)
    smp = random_colours(rng, n, nb * bs, 1.0)
    for i in range(0, n, 2):
        s, c = rng.integers(0, bs if i % 4 == 0 else nb * bs), rng.integers(0, 3)
        smp[i, s, c] = (np.nan, np.inf, -np.inf)[(i // 2) % 3]
    return Streams("nan_inf", smp, bs, 0.05, nb * bs - 1)


def negative_case(n=120, bs=4, nb=3, seed=19):
    """Negative luminance: the mean is negative, mean * mean is not."""
    rng = np.random.default_rng(seed)
    return Streams("negative", -random_colours(rng, n, nb * bs, 1.0), bs, 0.2, nb * bs - 1)


def bs1_case(n=150, nb=6, seed=23):
    """Batch size 1: the first test is 1 / 0 * 0 = NaN; half the pixels constant (converge at the second)."""
    rng = np.random.default_rng(seed)
    smp = random_colours(rng, n, nb, 1.0)
    smp[::2] = smp[::2, :1]
    return Streams("bs1", smp, 1, 0.3, nb - 1)


def mixed_case(n, bs, nb, seed):
    """Every kind of stream under one launch's settings: random colours at three scales, constant, black,
    NaN / inf, negative."""
    rng = np.random.default_rng(seed)
    S = nb * bs
    smp = random_colours(rng, n, S, 1.0)
    kind = rng.integers(0, 8, n)
    smp[kind == 0] *= 1e-3
    smp[kind == 1] *= 50.0
    smp[kind == 2] = smp[kind == 2][:, :1]
    smp[kind == 3] = 0.0
    smp[kind == 4] *= -1.0
    for i in np.flatnonzero(kind == 5):
        smp[i, rng.integers(0, S), rng.integers(0, 3)] = (np.nan, np.inf, -np.inf)[i % 3]
    # (the tolerance shrinks with the batch, so that about the same share converges per round at every size)
    return Streams("mixed_n%d_bs%d" % (n, bs), smp, bs, 0.1 / float(np.sqrt(bs)), S - 1)


_POOL = {}


def pool_streams(n, seed, short=False):
    """n <= 64 streams drawn from one pool of mixed streams (bs 4, three batches), for the shared layout
    cases of the round kernels -- the small frames have few real pixels.  short: max_samples 2 bs - 1, so
    whatever round 0 leaves stops in round 1; else 3 bs - 1, and most of it goes on.  A pool is folded
    once; a stream's fold does not depend on its neighbours."""
    if short not in _POOL:
        m = mixed_case(64, 4, 3, 606)
        _POOL[short] = Streams(m.name, m.samples, m.bs, m.tol, 2 * m.bs - 1 if short else m.max_samples)
    pool = _POOL[short]
    idx = np.random.default_rng(seed).permutation(pool.n)[:n]
    st = Streams("pool%d_n%d_s%d" % (short, n, seed), pool.samples[idx], pool.bs, pool.tol, pool.max_samples)
    st._fold = {k: v[idx] for k, v in pool.fold().items()}
    return st


def family_cases():
    return (threshold_cases() + [constant_case(), black_case()] + max_samples_cases() +
            [nan_inf_case(), negative_case(), bs1_case()])


def round_inputs(st, rnd):
    """What round `rnd` of a launch sees per the oracle: the streams still active (those that take more
    than rnd batches), and every stream's sums after round rnd - 1 (None for round 0)."""
    f = st.fold()
    active = np.flatnonzero(f["batches"] > rnd) if rnd < st.nb else np.zeros(0, dtype=np.int64)
    state = f["sums"][:, rnd - 1] if rnd else None
    return active, state


def round_partial(st, rnd, entries):
    """partial of a split round (sample-major): entry a's sample j at (j * n + a) * 3."""
    n = len(entries)
    blk = st.samples[entries, rnd * st.bs:(rnd + 1) * st.bs]  # [n, bs, 3]
    return np.ascontiguousarray(np.transpose(blk, (1, 0, 2))).reshape(-1)


def round_expect(st, rnd, entries):
    """Per entry of the segment: stops at this round?, sums after it, colour."""
    f = st.fold()
    stops = (f["batches"][entries] == rnd + 1) & (f["reason"][entries] != 3)
    return stops, f["sums"][entries, rnd], f["color"][entries]


def within_wave_rule(src, dst):
    """Survivors of each group of 64 consecutive entries of `src` appear in `dst` contiguously and in
    their original order (one atomic per wave; the order inside a wave is kept)."""
    where = {int(v): i for i, v in enumerate(src)}
    if len(where) != len(src) or any(int(v) not in where for v in dst):
        return False
    p = np.array([where[int(v)] for v in dst], dtype=np.int64)
    if len(p) == 0:
        return True
    g = p // 64
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    if len(set(g[starts].tolist())) != len(starts):
        return False  # a group split in two runs
    same = g[1:] == g[:-1]
    return bool((p[1:][same] > p[:-1][same]).all())


# ------------------------------------------------------------------ gs_round_resolve_kernel
def resolve_ref(lay, bs, conf, pstate, pbatches, want_out=True, want_out8=True):
    """(out, out8, map_samples, map_error, summary [active, sum of samples, max samples])."""
    real, _ = out_index(lay)
    word = pbatches.astype(np.int64)
    taken = (word & ~STOPPED & U32) * bs
    n = taken.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        colour = pstate[:, :3] / n[:, None]
        lsum, lsq = pstate[:, 3], pstate[:, 4]
        mean = lsum / n
        var = 1.0 / (n - 1.0) * (lsq - lsum * lsum / n)
        err = np.sqrt(conf * conf * var / n / (mean * mean))
    out, out8 = expected_outputs(lay, colour, np.ones(lay.cap, dtype=bool), want_out=want_out, want_out8=want_out8)
    ms = np.where(real, np.minimum(taken, U32), 0).astype(np.uint32)
    me = np.where(real, to_f32(err), np.float32(0.0)).astype(np.float32)
    act = int((real & ((word & STOPPED) == 0)).sum())
    summary = (act, int(taken[real].sum()), int(taken[real].max()) if real.any() else 0)
    return out, out8, ms, me, summary
