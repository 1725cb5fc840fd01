"""Device known-answer tests: the megakernel's own device functions (geometry.hpp,
devmath.hpp), run through the test-only harness tests/hip/kat_device.hip, against the
CPU oracle bit-for-bit on random and adversarial cases."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat(built):
    L = C.CDLL(os.path.join(HERE, "hip", "libkat_device.so"))
    P = C.c_void_p
    for f, args in {"kat_aabb": [C.c_int, P, P, P, P], "kat_aabb_cert": [C.c_int, P, P, P, P, P],
                    "kat_sphere": [C.c_int, P, P, P, P, P],
                    "kat_tri": [C.c_int, P, P, P, P], "kat_rng": [C.c_int, P, P, P, C.c_int, P],
                    "kat_math": [C.c_int, C.c_int, P, P, P],
                    "kat_noise": [C.c_int, C.c_int, P, C.c_double, P, P],
                    "kat_sky": [C.c_int, C.c_uint32, C.c_uint32, P, P],
                    "kat_rcp_cert": [C.c_int, P, P, P], "kat_div_by": [C.c_int, P, P, P, P]}.items():
        getattr(L, f).argtypes = args
        getattr(L, f).restype = C.c_int
    return L


def ptr(a):
    return a.ctypes.data


def _rays(rng, n, special=True):
    o = rng.uniform(-4, 4, (n, 3))
    d = rng.normal(size=(n, 3))
    if special:
        k = n // 4
        d[np.arange(k), rng.integers(0, 3, k)] = 0.0             # axis-parallel rays (1/0 = inf)
        d[k:2 * k, 0] = -0.0                                     # negative zero component
        o[2 * k:3 * k, 1] = np.round(o[2 * k:3 * k, 1])          # origins on integer planes
    return np.ascontiguousarray(np.hstack([o, d]))


def test_aabb_matches_oracle(kat):
    rng = np.random.default_rng(1)
    n = 20000
    ray = _rays(rng, n)
    lo = np.floor(rng.uniform(-3, 2, (n, 3)))
    ext = 1.0 + np.floor(rng.uniform(0, 3, (n, 3)))
    ext[rng.random(n) < 0.05, rng.integers(0, 3)] = 0.0                 # a few flat boxes
    box = np.ascontiguousarray(np.hstack([lo, lo + ext]))
    # aim 60% of the rays near their box (keeping the zero / negative-zero components) so
    # hits and misses are both common
    aim = rng.random(n) < 0.6
    to_box = 0.5 * (box[:, :3] + box[:, 3:]) - ray[:, :3] + rng.normal(scale=0.4, size=(n, 3))
    d = ray[:, 3:]
    ray[:, 3:] = np.where(aim[:, None] & (d != 0), to_box, d)
    iv = np.ascontiguousarray(np.stack([np.full(n, 0.001), np.where(rng.random(n) < 0.5, 1e300,
                                                                      rng.uniform(0, 6, n))], 1))
    out = np.zeros(n, np.int32)
    assert kat.kat_aabb(n, ptr(box), ptr(ray), ptr(iv), ptr(out)) == 0
    ref = np.array([oracle.aabb_hit(box[i, :3], box[i, 3:], ray[i, :3], ray[i, 3:], iv[i, 0], iv[i, 1])
                    for i in range(n)], np.int32)
    assert np.array_equal(out, ref)
    assert 0.05 < out.mean() < 0.95  # both outcomes exercised


def _grazing_cases(rng, n):
    """Rays aimed at box edges, faces and corners (tiny offsets, where f32 cannot decide),
    at unit and at C4 scales (boxes up to 2000 wide, origins up to 60 away)."""
    scale = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(1, 60, n))[:, None]
    lo = rng.uniform(-3, 2, (n, 3)) * scale
    ext = rng.uniform(0.01, 3, (n, 3)) * np.where(rng.random((n, 1)) < 0.1, 700.0, 1.0) * scale
    box = np.hstack([lo, lo + ext])
    o = rng.uniform(-6, 6, (n, 3)) * scale
    # a target on the box surface: a corner, an edge or a face point, nudged by +-ulps
    t = lo + ext * rng.integers(0, 2, (n, 3))
    face = rng.integers(0, 3, n)
    frac = rng.random((n, 3))
    for k in range(3):
        m = (face == k) & (rng.random(n) < 0.5)
        t[m, k] = lo[m, k] + ext[m, k] * frac[m, k]
    t = t * (1.0 + rng.choice([-1, 1], (n, 3)) * rng.choice([0.0, 1e-16, 1e-12, 1e-9, 1e-7, 1e-5], (n, 3)))
    d = t - o
    d = d / np.where(rng.random((n, 1)) < 0.5, 1.0, np.linalg.norm(d, axis=1, keepdims=True))
    ray = np.hstack([o, d])
    tmax = np.where(rng.random(n) < 0.6, 1.7976931348623157e308, rng.uniform(0.2, 3.0, n))
    iv = np.stack([np.full(n, 0.001), tmax], 1)
    return np.ascontiguousarray(box), np.ascontiguousarray(ray), np.ascontiguousarray(iv)


def test_certified_f32_slab_matches_oracle(kat):
    """The node test the kernel runs for cert rays (box_cert in f32, the f64 test where it
    is undecided) decides exactly as the reference's f64 AABB::hit, on random boxes and
    on rays grazing box corners / edges / faces by 1e-16 .. 1e-5 relative; every
    decision f32 certifies is correct, and undecided ones are rare on random rays."""
    rng = np.random.default_rng(11)
    n = 40000
    box, ray, iv = _grazing_cases(rng, n)
    # plus the random cases of test_aabb_matches_oracle (non-cert rays report -1)
    rb = rng.uniform(-3, 2, (n, 3))
    box = np.ascontiguousarray(np.vstack([box, np.hstack([rb, rb + rng.uniform(0.1, 3, (n, 3))])]))
    ray = np.ascontiguousarray(np.vstack([ray, _rays(rng, n)]))
    iv = np.ascontiguousarray(np.vstack([iv, np.stack([np.full(n, 0.001), rng.uniform(0, 6, n)], 1)]))
    m = 2 * n
    out = np.zeros(m, np.int32)
    dec = np.zeros(m, np.int32)
    assert kat.kat_aabb_cert(m, ptr(box), ptr(ray), ptr(iv), ptr(out), ptr(dec)) == 0
    ref = np.array([oracle.aabb_hit(box[i, :3], box[i, 3:], ray[i, :3], ray[i, 3:], iv[i, 0], iv[i, 1])
                    for i in range(m)], np.int32)
    cert = dec >= 0
    assert cert[:n].all() and 0.4 < cert[n:].mean() < 1.0  # grazing cases are cert rays; the zero / -0 direction cases are not
    assert np.array_equal(out[cert], ref[cert])
    sure = (dec == 0) | (dec == 1)
    assert np.array_equal(dec[sure], ref[sure])  # what f32 certifies is right
    assert (dec[:n] == 2).sum() > 50  # the grazing cases do reach the f64 fallback
    assert (dec[n:][cert[n:]] == 2).mean() < 1e-3  # and random rays almost never need it


def test_sphere_matches_oracle_bitwise(kat):
    from grayshift_amd._native import GS_OBJ_SPHERE
    rng = np.random.default_rng(2)
    n = 20000
    ray = _rays(rng, n)
    sph = np.ascontiguousarray(np.hstack([rng.uniform(-2, 2, (n, 3)), rng.uniform(0.1, 3, (n, 1))]))
    iv = np.ascontiguousarray(np.stack([np.full(n, 0.001), np.where(rng.random(n) < 0.7, 1e300,
                                                                      rng.uniform(0, 5, n))], 1))
    t = np.zeros(n)
    hit = np.zeros(n, np.int32)
    assert kat.kat_sphere(n, ptr(sph), ptr(ray), ptr(iv), ptr(t), ptr(hit)) == 0
    for i in range(n):
        h = oracle.prim_hit(GS_OBJ_SPHERE, sph[i], ray[i, :3], ray[i, 3:], iv[i, 0], iv[i, 1])
        assert (h is not None) == bool(hit[i]), i
        if h is not None:
            assert h["t"] == t[i], i  # sqrt and / are correctly rounded on both sides


@pytest.mark.parametrize("W,H", [(1024, 512), (4096, 2048), (7, 3)])
def test_certified_sky_index_equals_f64(kat, W, H):
    """sky_index_f32 (f32 atan2f angles, accepted only away from texel boundaries) gives the
    f64 path's texel column and row whenever it decides, on uniform directions and on
    directions within 1e-10 .. 1e-4 rad of column and row boundaries, and decides almost
    all uniform directions."""
    rng = np.random.default_rng(13)
    n = 1_000_000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    k = n // 2
    # near column boundaries: theta = 2 pi (i / W - 0.5) + delta; near row boundaries:
    # phi = pi (0.5 - j / H) + delta (the inverse of u, v in HDRI::sample)
    delta = np.where(rng.random(k) < 0.5, -1, 1) * 10.0 ** rng.uniform(-10, -4, k)
    th = 2 * np.pi * (rng.integers(0, W + 1, k) / W - 0.5) + delta
    ph = np.arcsin(np.clip(d[:k, 2], -1, 1))
    half = k // 2
    ph[:half] = np.pi * (0.5 - rng.integers(0, H + 1, half) / H) + delta[:half]
    th[:half] = rng.uniform(-np.pi, np.pi, half)
    d[:k] = np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], 1)
    d = np.ascontiguousarray(d)
    out = np.zeros((n, 4), np.int32)
    assert kat.kat_sky(n, W, H, ptr(d), ptr(out)) == 0
    dec = out[:, 0] >= 0
    assert np.array_equal(out[dec, :2], out[dec, 2:])
    # undecided share of uniform directions ~ 2 (1e-6 W + 2e-6 H): 0.4% for the 1024x512 sky
    assert dec[k:].mean() > 1.0 - 6e-6 * (W + H)
    assert (~dec[:k]).sum() > 1000  # the boundary cases do reach the f64 path


def test_triangle_matches_oracle_bitwise(kat):
    from grayshift_amd._native import GS_OBJ_TRIANGLE
    rng = np.random.default_rng(3)
    n = 20000
    ray = _rays(rng, n, special=False)
    tri = np.ascontiguousarray(rng.uniform(-2, 2, (n, 9)))
    aim = rng.random(n) < 0.6  # towards the centroid, so hits are common
    cen = (tri[:, 0:3] + tri[:, 3:6] + tri[:, 6:9]) / 3.0
    ray[aim, 3:] = cen[aim] - ray[aim, :3] + rng.normal(scale=0.3, size=(int(aim.sum()), 3))
    tuv = np.zeros((n, 3))
    hit = np.zeros(n, np.int32)
    assert kat.kat_tri(n, ptr(tri), ptr(ray), ptr(tuv), ptr(hit)) == 0
    for i in range(n):
        h = oracle.prim_hit(GS_OBJ_TRIANGLE, tri[i], ray[i, :3], ray[i, 3:], 0.001, 1e300)
        assert (h is not None) == bool(hit[i]), i
        if h is not None:
            assert (h["t"], h["u"], h["v"]) == tuple(tuv[i]), i
    assert 0.02 < hit.mean() < 0.9


def test_rng_streams_match_oracle(kat):
    rng = np.random.default_rng(4)
    n, draws = 4096, 24
    seed = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    pix = rng.integers(0, 2 ** 31, n).astype(np.uint32)
    smp = rng.integers(0, 5000, n).astype(np.uint32)
    out = np.zeros((n, draws))
    assert kat.kat_rng(n, ptr(seed), ptr(pix), ptr(smp), draws, ptr(out)) == 0
    for i in range(0, n, 7):
        f, _ = oracle.wyrand(oracle.stream_seed(int(seed[i]), int(pix[i]), int(smp[i])), draws)
        assert np.array_equal(out[i], f)


@pytest.mark.parametrize("which,fn,lo,hi", [(0, math.sin, 0.0, 2 * math.pi), (1, math.cos, 0.0, 2 * math.pi),
                                            (2, math.acos, -1.0, 1.0), (3, math.asin, -1.0, 1.0)])
def test_transcendentals_within_one_ulp_of_libm(kat, which, fn, lo, hi):
    """OCML vs glibc (what the reference's Rust f64::sin etc. call): never more than
    1 ulp apart on the ranges the path uses; the mismatch rate is the source of the
    rare traversal-counter differences."""
    rng = np.random.default_rng(5 + which)
    n = 50000
    x = np.ascontiguousarray(rng.uniform(lo, hi, n))
    out = np.zeros(n)
    assert kat.kat_math(n, which, ptr(x), None, ptr(out)) == 0
    ref = np.array([fn(v) for v in x])
    ulps = np.abs(out - ref) / np.spacing(np.abs(ref))
    assert ulps.max() <= 1.0
    print("which=%d mismatch rate %.4f" % (which, float((out != ref).mean())))


def test_perlin_matches_oracle_bitwise(kat):
    """NoiseTexture's Perlin (noise 0.9 restated, perlin.hpp) against the oracle's
    independent restatement: bit-identical (pure f64 + - * and floor)."""
    rng = np.random.default_rng(11)
    n = 20000
    p = rng.uniform(-300, 300, (n, 3))
    p[: n // 10] = np.round(p[: n // 10])          # lattice points (exactly 0)
    p[n // 10: n // 5] *= 1e-3                      # near the origin, both signs
    p = np.ascontiguousarray(p)
    perm = np.ascontiguousarray(oracle.noise_perm(0))
    out = np.zeros(n)
    assert kat.kat_noise(n, 0, ptr(perm), 0.0, ptr(p), ptr(out)) == 0
    ref = np.array([oracle.perlin3(q) for q in p])
    assert np.array_equal(out, ref)
    assert (out[: n // 10] == 0.0).all()


def test_noise_texture_value_within_libm_ulps(kat):
    """value_at = 0.5 * (1 + sin(scale * z + 10 * turbulence)): turbulence is bit-exact,
    sin is OCML vs glibc (<= 1 ulp), so the channel differs by at most a few ulps."""
    rng = np.random.default_rng(12)
    n = 5000
    p = np.ascontiguousarray(rng.uniform(-400, 600, (n, 3)))
    perm = np.ascontiguousarray(oracle.noise_perm(0))
    for scale in (4.0, 0.2):
        out = np.zeros(n)
        assert kat.kat_noise(n, 1, ptr(perm), scale, ptr(p), ptr(out)) == 0
        ref = np.array([oracle.noise_value(scale, q) for q in p])
        assert np.abs(out - ref).max() <= 4 * np.spacing(1.0)


def test_rcp_cert_within_the_certificates_bound(kat):
    """rcp_cert (geometry.hpp, round 6): the certified test's 1/d from the hardware reciprocal
    and two Newton steps must be within 2^-50 of the exact quotient over the cert range (|1/d|
    in [1e-25, 1e15]); outside it -- zeros, infinities, denormals -- it must give a value
    cert_ray_ok rejects (NaN, an infinity, or a magnitude out of range), never a finite
    in-range wrong one."""
    rng = np.random.default_rng(7)
    n = 400000
    mant = rng.uniform(1.0, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    d = mant * np.exp2(rng.integers(-83, 50, n)).astype(np.float64)
    d[:8] = [0.0, -0.0, np.inf, -np.inf, 5e-324, -1e-310, 1e-16, 1e26]
    d = np.ascontiguousarray(d)
    approx, exact = np.zeros(n), np.zeros(n)
    assert kat.kat_rcp_cert(n, ptr(d), ptr(approx), ptr(exact)) == 0
    with np.errstate(all="ignore"):
        inrange = (np.abs(exact) <= 1e15) & (np.abs(exact) >= 1e-25)
        rel = np.abs(approx[inrange] - exact[inrange]) / np.abs(exact[inrange])
        assert rel.max() <= 2.0 ** -50, rel.max()
        ok = lambda v: (np.abs(v) <= 1e15) & (np.abs(v) >= 1e-25)
        # a component clearly outside the range (zero, infinite, denormal, or 2x past a bound) is
        # rejected with the approximate value too; at a bound either choice is sound (the f64 test)
        out = ~((np.abs(exact) <= 2e15) & (np.abs(exact) >= 0.5e-25))
        assert out[:8].sum() >= 6 and not ok(approx[out]).any()


def test_root_division_through_the_reciprocal_is_exact(kat):
    """div_by (geometry.hpp, round 6: the sphere roots' (h -+ sqrt(disc)) / a through a refined
    reciprocal of a) equals the correctly rounded division bit for bit for every denominator in
    [2^-900, 2^900] and numerator >= 2^-968 in magnitude, incl. mantissas at the edges (all ones,
    powers of two), exact quotients and signed zeros' neighbours; a quotient under 2^-68 (below
    tmin) or an overflow may differ, and is rejected by the root's interval test either way."""
    rng = np.random.default_rng(11)
    n = 600000
    def draw(lo, hi, m):
        x = rng.uniform(1.0, 2.0, m) * np.exp2(rng.integers(lo, hi, m)).astype(np.float64)
        return np.where(rng.random(m) < 0.5, -x, x)
    den = np.abs(draw(-900, 900, n))
    num = draw(-968, 1000, n)
    k = n // 6  # edge mantissas: 1.111...1 and exact powers of two, exact small-integer quotients
    den[:k] = np.nextafter(np.exp2(rng.integers(-60, 60, k)).astype(np.float64), 0.0)
    num[k:2 * k] = np.exp2(rng.integers(-60, 60, k)).astype(np.float64)
    den[2 * k:3 * k] = rng.integers(1, 1 << 20, k).astype(np.float64)
    num[2 * k:3 * k] = den[2 * k:3 * k] * rng.integers(-1000, 1000, k)
    # the sphere's own shapes: a = |d|^2 of unit-ish directions, numerators h -+ sqrt(disc)
    den[3 * k:4 * k] = rng.uniform(0.01, 100.0, k)
    num[3 * k:4 * k] = rng.normal(scale=50.0, size=k)
    num, den = np.ascontiguousarray(num), np.ascontiguousarray(den)
    fast, exact = np.zeros(n), np.zeros(n)
    assert kat.kat_div_by(n, ptr(num), ptr(den), ptr(fast), ptr(exact)) == 0
    with np.errstate(all="ignore"):
        q = np.abs(num / den)
    inside = (q >= 2.0 ** -68) & np.isfinite(q) & (q < 1.7e308)
    assert inside.sum() > n // 2
    same = fast.view(np.uint64) == exact.view(np.uint64)
    assert same[inside].all(), (num[inside & ~same][:4], den[inside & ~same][:4])


# ---------------------------------------------------------------------------------------------
# The device functions below had no known-answer test: quad_accept, the leaf runs' sphere forms,
# box_hit_v / box_hit_fast, the instance transforms, reflect / refract, color_byte, the saturating
# casts, udiv, atan2 and sky_index_f64.  One thread per case, as above.
@pytest.fixture(scope="module")
def kat2(kat):
    P = C.c_void_p
    for f, args in {"kat_quad": [C.c_int, P, P, P, P, P], "kat_sphere_run": [C.c_int, C.c_int, P, P, P, P, P],
                    "kat_box": [C.c_int, C.c_int, P, P, P, P], "kat_inst": [C.c_int, P, P, P, P, P, P],
                    "kat_vec": [C.c_int, C.c_int, P, P, P, P], "kat_color_byte": [C.c_int, P, P],
                    "kat_sat": [C.c_int, C.c_int, P, P], "kat_udiv": [C.c_int, P, P, P]}.items():
        getattr(kat, f).argtypes = args
        getattr(kat, f).restype = C.c_int
    return kat


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _flat_quads():
    """The product's own flattened quad records (q, u, v, then the host's w, normal and D: 17
    doubles each with the material word) of a scene of random, axis-aligned and sliver quads."""
    import grayshift_amd as g
    rng = np.random.default_rng(21)
    b = g.SceneBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    # power-of-two axis-aligned quads: alpha and beta are exact, so edges and corners are hit exactly
    b.add(b.quad((0, 0, 0), (2, 0, 0), (0, 0, 4), m))
    b.add(b.quad((-4, 1, -2), (0, 0, 8), (0, 2, 0), m))
    b.add(b.quad((1, -1, 3), (0, 4, 0), (0.5, 0, 0), m))
    for _ in range(40):
        q, u, v = rng.uniform(-3, 3, 3), rng.normal(size=3), rng.normal(size=3)
        b.add(b.quad(q, u * rng.uniform(0.2, 3), v * rng.uniform(0.2, 3), m))
    for _ in range(8):  # slivers: u and v nearly parallel
        q, u = rng.uniform(-3, 3, 3), rng.normal(size=3)
        b.add(b.quad(q, u, u * rng.uniform(0.5, 2) + rng.normal(size=3) * 1e-3, m))
    host = g.HostScene(b.build())
    try:
        n = host.flat.n_quads
        assert n == 51 and C.sizeof(C.c_double) * 17 == 136
        return np.ctypeslib.as_array((C.c_double * (17 * n)).from_address(host.flat.quads)).reshape(n, 17).copy()
    finally:
        host.close()


def test_quad_accept_matches_oracle_bitwise(kat2):
    """quad_accept on the host's records (normal, D, w) against Quad::hit of the oracle, which
    derives them itself from q, u, v: hit flag and t.  Random rays at and around the quads; rays
    exactly onto edges and corners (alpha, beta in {0, 1}: the closed interval) with zero and -0
    direction components; rays parallel to the plane; |normal . d| from 1e-9 to 1e-7 with the hit
    point inside the quad (so the 1e-8 threshold alone decides); t == tmin and t == tmax (closed)
    and one ulp outside."""
    from grayshift_amd._native import GS_OBJ_QUAD
    rng = np.random.default_rng(22)
    Q = _flat_quads()
    nq = len(Q)
    # the three power-of-two axis-aligned quads, wherever the flattening put them
    exact = [int(np.flatnonzero((Q[:, 3:9] == uv).all(1))[0])
             for uv in ((2, 0, 0, 0, 0, 4), (0, 0, 8, 0, 2, 0), (0, 4, 0, 0.5, 0, 0))]
    BIG = 1e300

    def at(idx, a, bta):
        return Q[idx, 0:3] + a[:, None] * Q[idx, 3:6] + bta[:, None] * Q[idx, 6:9]

    idx, ray, iv = [], [], []
    # (a) random rays aimed at and around the quads, unnormalised
    n = 9000
    i = rng.integers(0, nq, n)
    o = rng.uniform(-6, 6, (n, 3))
    d = (at(i, rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 1.2, n)) - o) * rng.uniform(0.1, 3, (n, 1))
    idx.append(i); ray.append(np.hstack([o, d]))
    iv.append(np.stack([np.full(n, 0.001), np.where(rng.random(n) < 0.5, BIG, rng.uniform(0, 4, n))], 1))
    # (b) straight down the normal of the three exact quads onto corners, edges, inside and just
    # outside: alpha, beta in {0, 1/2, 1, -1/4, 5/4}; the ray's other components are 0 or -0
    ex = []
    for qi in exact:
        nrm = Q[qi, 12:15]
        for a in (0.0, 0.5, 1.0, -0.25, 1.25):
            for bt in (0.0, 0.5, 1.0, -0.25, 1.25):
                for zero in (0.0, -0.0):
                    p = Q[qi, 0:3] + a * Q[qi, 3:6] + bt * Q[qi, 6:9]
                    dd = np.where(nrm != 0, -nrm * 2.0, zero)
                    ex.append((qi, np.hstack([p + nrm * 4.0, dd]), a, bt))
    n_b = len(ex)
    idx.append(np.array([e[0] for e in ex])); ray.append(np.array([e[1] for e in ex]))
    iv.append(np.tile([0.001, BIG], (n_b, 1)))
    inside_b = np.array([0.0 <= e[2] <= 1.0 and 0.0 <= e[3] <= 1.0 for e in ex])
    # (c) parallel rays: d in the plane (exactly, for the exact quads; to rounding for the others)
    n = 1000
    i = np.concatenate([np.array(exact)[rng.integers(0, 3, n // 2)], rng.integers(0, nq, n // 2)])
    d = rng.normal(size=(n, 1)) * Q[i, 3:6] + rng.normal(size=(n, 1)) * Q[i, 6:9]
    d[: n // 4] = Q[i[: n // 4], 3:6]
    d[: n // 8][d[: n // 8] == 0] = -0.0
    idx.append(i); ray.append(np.hstack([rng.uniform(-3, 3, (n, 3)), d])); iv.append(np.tile([0.001, BIG], (n, 1)))
    # (d) |den| around 1e-8: d = tangent + s * normal, the origin one step of d before a point
    # inside the quad, so the ray reaches that point at t ~ 1 whenever the den test lets it
    n = 4000
    i = rng.integers(0, nq, n)
    s = 10.0 ** rng.uniform(-9, -7, n) * rng.choice([-1.0, 1.0], n)
    s[:400] = 1e-8 * (1.0 + rng.uniform(-1e-6, 1e-6, 400)) * rng.choice([-1.0, 1.0], 400)
    tang = Q[i, 3:6] / np.linalg.norm(Q[i, 3:6], axis=1, keepdims=True)
    d = tang + s[:, None] * Q[i, 12:15]
    p = at(i, rng.uniform(0.3, 0.7, n), rng.uniform(0.3, 0.7, n))
    idx.append(i); ray.append(np.hstack([p - d, d])); iv.append(np.tile([0.001, BIG], (n, 1)))
    n_d0 = sum(len(x) for x in idx) - n
    idx, ray, iv = np.concatenate(idx), np.vstack(ray), np.vstack(iv)
    # (e) the interval's ends: the first 1200 hits of (a) again with tmin = t, tmax = t and one ulp outside
    t_a = [oracle.prim_hit(GS_OBJ_QUAD, Q[idx[k], :9], ray[k, :3], ray[k, 3:], 0.0, BIG) for k in range(3000)]
    hits = [k for k in range(3000) if t_a[k] is not None and t_a[k]["t"] > 1e-6][:1200]
    assert len(hits) == 1200
    t = np.array([t_a[k]["t"] for k in hits])
    ends = np.vstack([np.stack([t, np.full_like(t, BIG)], 1), np.stack([np.nextafter(t, np.inf), np.full_like(t, BIG)], 1),
                      np.stack([np.zeros_like(t), t], 1), np.stack([np.zeros_like(t), np.nextafter(t, -np.inf)], 1)])
    n_e0 = len(idx)
    idx = np.concatenate([idx] + [idx[hits]] * 4)
    ray = np.vstack([ray] + [ray[hits]] * 4)
    iv = np.vstack([iv, ends])

    n = len(idx)
    assert n <= 20000
    quads = np.ascontiguousarray(Q[idx])
    ray, iv = np.ascontiguousarray(ray), np.ascontiguousarray(iv)
    tt, hit = np.zeros(n), np.zeros(n, np.int32)
    assert quads.shape == (n, 17) and ray.shape == (n, 6) and iv.shape == (n, 2)
    assert kat2.kat_quad(n, ptr(quads), ptr(ray), ptr(iv), ptr(tt), ptr(hit)) == 0
    ref = np.zeros(n, np.int32)
    for k in range(n):
        h = oracle.prim_hit(GS_OBJ_QUAD, Q[idx[k], :9], ray[k, :3], ray[k, 3:], iv[k, 0], iv[k, 1])
        ref[k] = h is not None
        assert ref[k] == hit[k], k
        if h is not None:
            assert h["t"] == tt[k], k
    assert 0.2 < ref[:9000].mean() < 0.9
    b0 = 9000
    assert np.array_equal(ref[b0:b0 + n_b].astype(bool), inside_b)  # edges and corners are inside (closed)
    assert not ref[b0 + n_b:b0 + n_b + 250].any()                   # exactly parallel: den == 0
    dd = ref[n_d0:n_e0]
    assert 0.3 < dd.mean() < 0.7 and 0.2 < dd[:400].mean() < 0.8    # both sides of 1e-8
    e = ref[n_e0:].reshape(4, -1)
    assert e[0].all() and e[2].all() and not e[1].any() and not e[3].any()  # closed ends


_SPHERE_CASES = {}


def _sphere_cases():
    """(sph, ray, iv, oracle hit, oracle t), made once: the cases of test_sphere_matches_oracle_
    bitwise plus tangent rays (discriminant within a few ulps of 0, both sides), origins inside
    the sphere, unnormalised directions with a = |d|^2 from 1e-6 to 1e6, and roots exactly at
    the (open) interval's ends."""
    if _SPHERE_CASES:
        return _SPHERE_CASES["c"]
    from grayshift_amd._native import GS_OBJ_SPHERE
    rng = np.random.default_rng(31)
    n = 4000
    ray = _rays(rng, n)
    sph = np.hstack([rng.uniform(-2, 2, (n, 3)), rng.uniform(0.1, 3, (n, 1))])
    iv = np.stack([np.full(n, 0.001), np.where(rng.random(n) < 0.7, 1e300, rng.uniform(0, 5, n))], 1)
    # tangent: the centre at distance r (1 + delta) from the ray's line
    m = 4000
    o = rng.uniform(-4, 4, (m, 3))
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perp = np.cross(d, rng.normal(size=(m, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    r = rng.uniform(0.1, 3, m)
    delta = rng.choice([0.0, 1e-16, 2e-16, 1e-15, 1e-14, 1e-12, 1e-9], m) * rng.choice([-1.0, 1.0], m)
    c = o + d * rng.uniform(0.5, 6, (m, 1)) + perp * (r * (1.0 + delta))[:, None]
    d *= np.where(rng.random((m, 1)) < 0.5, 1.0, rng.uniform(0.2, 5, (m, 1)))
    ray = np.vstack([ray, np.hstack([o, d])])
    sph = np.vstack([sph, np.hstack([c, r[:, None]])])
    iv = np.vstack([iv, np.tile([0.001, 1e300], (m, 1))])
    # inside the sphere, and |d|^2 from 1e-6 to 1e6
    m = 4000
    c = rng.uniform(-2, 2, (m, 3))
    r = rng.uniform(0.1, 3, m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.where(rng.random((m, 1)) < 0.5, c + u * (r * rng.uniform(0, 0.999, m))[:, None], rng.uniform(-4, 4, (m, 3)))
    d = (c + rng.normal(scale=0.7, size=(m, 3)) * r[:, None] - o)
    d *= (10.0 ** rng.uniform(-3, 3, (m, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    ray = np.vstack([ray, np.hstack([o, d])])
    sph = np.vstack([sph, np.hstack([c, r[:, None]])])
    iv = np.vstack([iv, np.stack([np.full(m, 0.001), np.where(rng.random(m) < 0.7, 1e300, rng.uniform(0, 5, m))], 1)])
    a = (ray[:, 3:] ** 2).sum(1)
    assert a[-m:].min() < 1e-5 and a[-m:].max() > 1e5

    def run(sph, ray, iv):
        hit, t = np.zeros(len(sph), np.int32), np.zeros(len(sph))
        for k in range(len(sph)):
            h = oracle.prim_hit(GS_OBJ_SPHERE, sph[k], ray[k, :3], ray[k, 3:], iv[k, 0], iv[k, 1])
            hit[k] = h is not None
            t[k] = h["t"] if h is not None else 0.0
        return hit, t

    hit, t = run(sph, ray, iv)
    # roots at the ends: hits again with tmin = t (the near root is excluded: the far one or a
    # miss) and tmax = t (excluded: a miss, both roots), and one ulp inside
    k = np.flatnonzero((hit == 1) & (iv[:, 1] == 1e300))[:1500]
    tk = t[k]
    ends = np.vstack([np.stack([tk, np.full_like(tk, 1e300)], 1), np.stack([np.full_like(tk, 0.001), tk], 1),
                      np.stack([np.nextafter(tk, -np.inf), np.full_like(tk, 1e300)], 1),
                      np.stack([np.full_like(tk, 0.001), np.nextafter(tk, np.inf)], 1)])
    hit2, t2 = run(np.vstack([sph[k]] * 4), np.vstack([ray[k]] * 4), ends)
    e = hit2.reshape(4, -1)
    assert not e[1].any() and e[2].all() and e[3].all() and (t2.reshape(4, -1)[0][e[0] == 1] > tk[e[0] == 1]).all()
    sph, ray, iv = np.vstack([sph] + [sph[k]] * 4), np.vstack([ray] + [ray[k]] * 4), np.vstack([iv, ends])
    hit, t = np.concatenate([hit, hit2]), np.concatenate([t, t2])
    assert len(sph) <= 20000 and 0.2 < hit.mean() < 0.9
    tang = hit[4000:8000]
    assert 0.2 < tang.mean() < 0.8  # both sides of the tangent
    _SPHERE_CASES["c"] = tuple(np.ascontiguousarray(x) for x in (sph, ray, iv, hit, t))
    return _SPHERE_CASES["c"]


@pytest.mark.parametrize("which,name", [(-1, "sphere_accept"), (0, "sphere_accept_rr_ra"),
                                        (1, "sphere_disc_rr + sphere_root_take"),
                                        (2, "sphere_disc_rr + sphere_root_take_ra")])
def test_leaf_run_sphere_forms_match_oracle_bitwise(kat2, which, name):
    """What the leaf runs execute (geometry.hpp): the whole test with the roots' divisions through
    rcp_cert(a), and the test split at the discriminant with either division: hit flag and t equal
    Sphere::hit's of the oracle bit for bit (sphere_accept itself on the same cases too)."""
    sph, ray, iv, ref_hit, ref_t = _sphere_cases()
    n = len(sph)
    t, hit = np.zeros(n), np.zeros(n, np.int32)
    if which < 0:
        assert kat2.kat_sphere(n, ptr(sph), ptr(ray), ptr(iv), ptr(t), ptr(hit)) == 0
    else:
        assert kat2.kat_sphere_run(n, which, ptr(sph), ptr(ray), ptr(iv), ptr(t), ptr(hit)) == 0
    bad = np.flatnonzero(hit != ref_hit)
    assert bad.size == 0, (name, bad[:5])
    h = ref_hit == 1
    bad = np.flatnonzero(_bits(t[h]) != _bits(ref_t[h]))
    assert bad.size == 0, (name, bad[:5], t[h][bad[:5]], ref_t[h][bad[:5]])


_BOX_CASES = {}


def _box_cases():
    """(box, ray, iv, oracle decision): 10000 random cases as test_aabb_matches_oracle's (zero and
    -0 direction components, origins on slab planes, flat boxes) and 10000 grazing ones."""
    if _BOX_CASES:
        return _BOX_CASES["c"]
    rng = np.random.default_rng(41)
    n = 10000
    ray = _rays(rng, n)
    lo = np.floor(rng.uniform(-3, 2, (n, 3)))
    ext = 1.0 + np.floor(rng.uniform(0, 3, (n, 3)))
    ext[rng.random(n) < 0.05, rng.integers(0, 3)] = 0.0
    box = np.hstack([lo, lo + ext])
    aim = rng.random(n) < 0.6
    to_box = 0.5 * (box[:, :3] + box[:, 3:]) - ray[:, :3] + rng.normal(scale=0.4, size=(n, 3))
    d = ray[:, 3:]
    ray[:, 3:] = np.where(aim[:, None] & (d != 0), to_box, d)
    iv = np.stack([np.full(n, 0.001), np.where(rng.random(n) < 0.5, 1e300, rng.uniform(0, 6, n))], 1)
    gb, gr, gi = _grazing_cases(rng, n)
    box, ray, iv = (np.ascontiguousarray(np.vstack(p)) for p in ((box, gb), (ray, gr), (iv, gi)))
    ref = np.array([oracle.aabb_hit(box[i, :3], box[i, 3:], ray[i, :3], ray[i, 3:], iv[i, 0], iv[i, 1])
                    for i in range(2 * n)], np.int32)
    assert 0.1 < ref.mean() < 0.9
    _BOX_CASES["c"] = (box, ray, iv, ref)
    return _BOX_CASES["c"]


@pytest.mark.parametrize("which,name", [(0, "box_hit"), (1, "box_hit_v"), (2, "box_hit_fast")])
def test_box_forms_match_oracle(kat2, which, name):
    """box_hit_v (the nested walk's per-lane interval) decides every case as AABB::hit of the
    oracle and as box_hit; box_hit_fast (min / max in the swap's place) every case where
    fast_slab_ray holds, which is where the megakernel calls it."""
    box, ray, iv, ref = _box_cases()
    n = len(ref)
    out = np.zeros(n, np.int32)
    assert kat2.kat_box(n, which, ptr(box), ptr(ray), ptr(iv), ptr(out)) == 0
    if which == 2:
        fast = out >= 0
        assert fast[n // 2:].all() and 0.3 < fast[: n // 2].mean() < 0.9  # grazing: all; zero / -0 components: not
        assert (out[fast] == 1).any() and (out[fast] == 0).any()
        assert np.array_equal(out[fast], ref[fast])
    else:
        assert np.array_equal(out, ref)


def test_instance_transforms_match_f64_bitwise(kat2):
    """inst_forward / inst_backward (hittable.rs:107-117, :179-207) over chains of up to three
    Translate / RotateY instances, against numpy f64 with the same expressions in the same order
    (sums and products only: bit for bit); sin and cos are inputs.  The first quarter of the
    cases are full chains of three: forward outermost first, backward innermost first."""
    rng = np.random.default_rng(51)
    n = 20000
    kind = rng.integers(0, 3, (n, 3)).astype(np.int32)
    kind[: n // 4] = rng.integers(1, 3, (n // 4, 3))
    th = rng.uniform(-np.pi, np.pi, (n, 3))
    th[rng.random((n, 3)) < 0.1] = 0.0
    par = np.where((kind == 1)[:, :, None], rng.uniform(-5, 5, (n, 3, 3)),
                   np.stack([np.sin(th), np.cos(th), np.zeros((n, 3))], 2))
    ray = rng.normal(size=(n, 6)) * 3
    ray[rng.random((n, 6)) < 0.05] = 0.0
    ray[rng.random((n, 6)) < 0.02] = -0.0
    pn = rng.normal(size=(n, 6))
    kind, par, ray, pn = (np.ascontiguousarray(x) for x in (kind, par.reshape(n, 9), ray, pn))
    ro, po = np.zeros((n, 6)), np.zeros((n, 6))
    assert kat2.kat_inst(n, ptr(kind), ptr(par), ptr(ray), ptr(pn), ptr(ro), ptr(po)) == 0

    o, d = ray[:, :3].copy(), ray[:, 3:].copy()
    for k in range(3):
        p = par[:, 3 * k:3 * k + 3]
        s, c = p[:, 0], p[:, 1]
        tr, rot = (kind[:, k] == 1)[:, None], (kind[:, k] == 2)[:, None]
        fwd = lambda v: np.stack([(c * v[:, 0]) - (s * v[:, 2]), v[:, 1], (s * v[:, 0]) + (c * v[:, 2])], 1)
        o, d = np.where(tr, o - p, np.where(rot, fwd(o), o)), np.where(rot, fwd(d), d)
    p_, n_ = pn[:, :3].copy(), pn[:, 3:].copy()
    for k in (2, 1, 0):
        p = par[:, 3 * k:3 * k + 3]
        s, c = p[:, 0], p[:, 1]
        tr, rot = (kind[:, k] == 1)[:, None], (kind[:, k] == 2)[:, None]
        bwd = lambda v: np.stack([(c * v[:, 0]) + (s * v[:, 2]), v[:, 1], ((-s) * v[:, 0]) + (c * v[:, 2])], 1)
        p_, n_ = np.where(tr, p_ + p, np.where(rot, bwd(p_), p_)), np.where(rot, bwd(n_), n_)
    assert np.array_equal(_bits(ro), _bits(np.hstack([o, d])))
    assert np.array_equal(_bits(po), _bits(np.hstack([p_, n_])))
    assert not np.array_equal(ro[: n // 4], ray[: n // 4])


def test_reflect_and_refract_match_bitwise(kat2):
    """reflect (vec3.rs:53-55) against numpy f64 in the reference's order; refract (vec3.rs:57-62)
    against the oracle's, incl. grazing directions at ratio > 1 where 1 - |perp|^2 is negative
    (the fabs branch) and cos_theta clamped by the min."""
    rng = np.random.default_rng(61)
    n = 20000
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    k = n // 4  # grazing: v nearly perpendicular to n
    v[:k] = np.cross(nr[:k], rng.normal(size=(k, 3)))
    v[:k] /= np.linalg.norm(v[:k], axis=1, keepdims=True)
    v[:k] -= nr[:k] * rng.uniform(0, 0.2, (k, 1))
    v[k:k + 100] = -nr[k:k + 100] * (1.0 + 1e-15)  # dot(n, -v) just above 1: the min
    v[k + 100:k + 200] *= 3.0                        # not unit
    ratio = rng.choice([1.5, 1.0 / 1.5, 2.4, 1.0, 1.0 / 1.33], n)
    v, nr, ratio = np.ascontiguousarray(v), np.ascontiguousarray(nr), np.ascontiguousarray(ratio)
    out = np.zeros((n, 3))
    assert kat2.kat_vec(n, 0, ptr(v), ptr(nr), ptr(ratio), ptr(out)) == 0
    dot = v[:, 0] * nr[:, 0] + v[:, 1] * nr[:, 1] + v[:, 2] * nr[:, 2]
    assert np.array_equal(_bits(out), _bits(v - nr * (2.0 * dot)[:, None]))
    assert kat2.kat_vec(n, 1, ptr(v), ptr(nr), ptr(ratio), ptr(out)) == 0
    ref = np.array([oracle.refract(v[i], nr[i], ratio[i]) for i in range(n)])
    assert np.array_equal(_bits(out), _bits(ref))
    cos = np.minimum(-dot, 1.0)
    perp2 = (((v + nr * cos[:, None]) * ratio[:, None]) ** 2).sum(1)
    assert (perp2 > 1.0).sum() > 500 and (perp2 < 1.0).sum() > 5000 and (-dot > 1.0).sum() >= 50


def test_color_byte_matches_oracle(kat2):
    """write_color's byte (color.rs:8-28): both neighbours of every byte boundary (k / 256)^2, and
    a few ulps around; 0, -0, negatives, denormals; the 0.999 clamp; +-inf and NaN."""
    c = []
    for k in range(1, 257):
        x = (k / 256.0) ** 2
        c += [x, np.nextafter(x, 0.0), np.nextafter(x, 4.0), np.nextafter(np.nextafter(x, 0.0), 0.0),
              np.nextafter(np.nextafter(x, 4.0), 4.0)]
    top = 0.999 ** 2
    c += [0.0, -0.0, -1e-300, -1.0, -np.inf, 5e-324, 1e-310, 1e-12, top, np.nextafter(top, 0.0), np.nextafter(top, 4.0),
          0.998 ** 2, 1.0, 1.0000001, 2.0, 65536.0, 1e300, np.inf, np.nan]
    c += list(np.random.default_rng(71).uniform(0, 1.2, 2000))
    c = np.ascontiguousarray(c, dtype=np.float64)
    out = np.zeros(len(c), np.int32)
    assert kat2.kat_color_byte(len(c), ptr(c), ptr(out)) == 0
    ref = np.array([oracle.color_byte(float(x)) for x in c], np.int32)
    assert np.array_equal(out, ref)
    assert set(ref.tolist()) == set(range(256))  # every byte value occurs; 255 is the clamp's


def test_saturating_casts_match_rust(kat2):
    """sat_i32 is Rust's `f64 as i32` and sat_u64 its `as u64` / `as u32`: truncation toward
    zero, saturation at the type's ends, NaN -> 0."""
    edges = []
    for p in (2.0 ** 31, 2.0 ** 32, 2.0 ** 63, 2.0 ** 64, 2147483647.0, 4294967295.0, 1.0, 0.0):
        for s in (1.0, -1.0):
            x = s * p
            edges += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf), x + 0.5, x - 0.5, x + 1.0, x - 1.0]
    edges += [-0.0, 0.9999999999999999, -0.9999999999999999, 1e300, -1e300, np.inf, -np.inf, np.nan, 5e-324]
    rng = np.random.default_rng(81)
    f = np.concatenate([edges, rng.normal(size=2000) * 10.0 ** rng.uniform(-2, 22, 2000)])
    f = np.ascontiguousarray(f)

    def rust(x, lo, hi):
        if x != x:
            return 0
        if x == np.inf:
            return hi
        if x == -np.inf:
            return lo
        return max(lo, min(hi, int(x)))  # int(): toward zero, exact for any finite double

    for which, lo, hi in ((0, -2 ** 31, 2 ** 31 - 1), (1, 0, 2 ** 64 - 1), (2, 0, 2 ** 32 - 1)):
        out = np.zeros(len(f), np.uint64)
        assert kat2.kat_sat(len(f), which, ptr(f), ptr(out)) == 0
        ref = np.array([rust(float(x), lo, hi) % 2 ** 64 for x in f], np.uint64)
        bad = np.flatnonzero(out != ref)
        assert bad.size == 0, (which, f[bad[:5]], out[bad[:5]], ref[bad[:5]])


def test_udiv_equals_floor_division(kat2):
    """udiv(n, udiv_make(d)) == n // d (the launches' fixed divisors: image width, tiles per row,
    chunks per pixel): the divisors' ends and n at 0, d - 1, d, multiples of d and their
    neighbours, 2^32 - 1, plus random pairs."""
    rng = np.random.default_rng(91)
    ds = [1, 2, 3, 5, 7, 64, 1920, 65535, 65537, 2 ** 31, 2 ** 32 - 1]
    ds += [int(x) for x in rng.integers(1, 2 ** 32, 300)] + [int(x) for x in rng.integers(1, 5000, 300)]
    num, den = [], []
    for d in ds:
        ns = [0, d - 1, d, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]
        top = (2 ** 32 - 1) // d
        for k in {1, 2, 3, top // 2, max(top - 1, 0), top} | {int(x) for x in rng.integers(0, top + 1, 8)}:
            ns += [k * d - 1, k * d, k * d + 1]
        ns += [int(x) for x in rng.integers(0, 2 ** 32, 24)]
        ns = [x for x in ns if 0 <= x < 2 ** 32]
        num += ns
        den += [d] * len(ns)
    num, den = np.array(num, np.uint32), np.array(den, np.uint32)
    out = np.zeros(len(num), np.uint32)
    assert kat2.kat_udiv(len(num), ptr(num), ptr(den), ptr(out)) == 0
    ref = (num.astype(np.uint64) // den.astype(np.uint64)).astype(np.uint32)
    bad = np.flatnonzero(out != ref)
    assert bad.size == 0, (num[bad[:5]], den[bad[:5]], out[bad[:5]], ref[bad[:5]])


def test_atan2_within_one_ulp_of_libm(kat2):
    """OCML atan2 vs glibc on sphere_uv's atan2(-p.z, p.x) and the sky's atan2(y, x): components of
    unit vectors in every quadrant, near and on the axes, with signed zeros."""
    rng = np.random.default_rng(9)
    n = 50000
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    y, x = -p[:, 2].copy(), p[:, 0].copy()
    k = 4000
    y[:k] = 10.0 ** rng.uniform(-40, -1, k) * rng.choice([-1.0, 1.0], k)   # next to the x axis
    x[k:2 * k] = 10.0 ** rng.uniform(-40, -1, k) * rng.choice([-1.0, 1.0], k)  # next to the y axis
    ax = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0),
          (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0)]
    y[2 * k:2 * k + len(ax)] = [a[0] for a in ax]
    x[2 * k:2 * k + len(ax)] = [a[1] for a in ax]
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    out = np.zeros(n)
    assert kat2.kat_math(n, 4, ptr(y), ptr(x), ptr(out)) == 0
    ref = np.array([math.atan2(a, b) for a, b in zip(y, x)])
    ulps = np.abs(out - ref) / np.spacing(np.abs(ref))
    assert ulps.max() <= 1.0, (y[ulps.argmax()], x[ulps.argmax()])
    print("atan2 mismatch rate %.4f" % float((out != ref).mean()))


@pytest.mark.parametrize("W,H", [(1024, 512), (8, 4), (7, 3)])
def test_sky_index_f64_matches_the_formula(kat2, W, H):
    """sky_index_f64 (HDRI::sample's texel column and row, camera.rs:257-270) against the same
    formula in numpy f64, for directions farther than 1e-9 rad from a texel boundary (closer, an
    ulp of atan2 / asin decides): uniform directions, directions 1e-8 .. 1e-4 rad from column and
    row boundaries, the poles, the axes and the seam at theta = +-pi."""
    rng = np.random.default_rng(14)
    n = 200000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    k = n // 2
    delta = np.where(rng.random(k) < 0.5, -1, 1) * 10.0 ** rng.uniform(-8, -4, k)
    th = 2 * np.pi * (rng.integers(0, W + 1, k) / W - 0.5) + delta
    ph = np.arcsin(np.clip(d[:k, 2], -1, 1))
    half = k // 2
    ph[:half] = np.clip(np.pi * (0.5 - rng.integers(0, H + 1, half) / H) + delta[:half], -np.pi / 2, np.pi / 2)
    th[:half] = rng.uniform(-np.pi, np.pi, half)
    d[:k] = np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], 1)
    d[k:k + 8] = [(1, 0, 0), (-1, 0.0, 0), (-1, -0.0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-1, 1e-12, 0)]
    d = np.ascontiguousarray(d)
    out = np.zeros((n, 4), np.int32)
    assert kat2.kat_sky(n, W, H, ptr(d), ptr(out)) == 0
    theta, phi = np.arctan2(d[:, 1], d[:, 0]), np.arcsin(d[:, 2])
    uW, vH = (0.5 + theta / (2.0 * np.pi)) * W, (0.5 - phi / np.pi) * H
    x = np.floor(np.maximum(uW, 0.0)).astype(np.uint64) % W
    y = np.floor(np.maximum(vH, 0.0)).astype(np.uint64) % H
    # distance to the nearest texel boundary in radians: a column is 2 pi / W wide, a row pi / H
    far = (np.abs(uW - np.round(uW)) * (2 * np.pi / W) > 1e-9) & (np.abs(vH - np.round(vH)) * (np.pi / H) > 1e-9)
    assert far.mean() > 0.9 and far[:k].mean() > 0.8  # (a boundary row clipped to a pole is on it)
    assert np.array_equal(out[far, 2], x[far].astype(np.int32))
    assert np.array_equal(out[far, 3], y[far].astype(np.int32))
    assert len(np.unique(out[far, 2])) == W and len(np.unique(out[far, 3])) == H
