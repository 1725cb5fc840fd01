"""The cases of the shading known-answer tests (tests/shade_cases.py) reach the edges they are
there for: asserted on the oracle's answers alone, so this runs without a device.  The device
test (tests/test_gpu_shading_kat.py) compares the same cases bit for bit; a branch that no case
takes would pass there unseen."""
import numpy as np
import pytest

import grayshift_amd as g

import oracle

from tests import shade_cases as S

ULP1 = 2.0 ** -52  # the spacing of doubles in [1, 2)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _mixed():
    return S.scene("mixed"), S.cases("mixed"), S.answers("mixed")


def _is(c, *labels):
    return np.isin(c["label"], labels)


# ------------------------------------------------------------------ scenes and their leaves
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_every_object_is_found_in_the_flat_scene(name):
    """Each object's leaf (and so the refs a hit on it carries) is found by its anchor, each
    with a flat material of its own; the oracle reports the object's spec material."""
    sc, c, a = S.scene(name), S.cases(name), S.answers(name)
    hs = g.HostScene(sc.spec)
    leaves = S.flat_leaves(hs.flat)
    mats = [leaves[o.anchor][3] for o in sc.objs]
    assert len(set(mats)) == len(mats)
    hit = a["hit"]
    assert np.array_equal(a["mat"][hit], np.array([o.mat for o in sc.objs])[c["k"][hit]])
    if name == "deep":
        by = {o.label: leaves[o.anchor] for o in sc.objs}
        chain = lambda ref: S.REF_INST == ref >> S.REF_SHIFT  # noqa: E731
        assert chain(by["chain6"][1]) and by["chain6"][2] == S.REF_NONE
        assert chain(by["chain3_in_bvh_chain2"][1]) and chain(by["chain3_in_bvh_chain2"][2])
        assert chain(by["plain_in_bvh_chain3"][1]) and by["plain_in_bvh_chain3"][2] == S.REF_NONE
    hs.close()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_few_aimed_rays_miss_and_launches_stay_small(name):
    c, a = S.cases(name), S.answers(name)
    aimed = c["k"] >= 0
    assert (~a["hit"][aimed]).mean() <= 0.10
    assert len(c["k"]) <= 2 * S.LAUNCH
    assert (~aimed).sum() >= 64  # miss lanes


def test_every_wave_of_the_mixed_scene_holds_every_kind_of_lane():
    _, c, a = _mixed()
    lab = c["label"]
    kinds = [np.char.startswith(lab, "lamb"), np.char.startswith(lab, "metal"), np.char.startswith(lab, "diel"),
             np.char.startswith(lab, "medium"), np.char.startswith(lab, "light"), lab == "miss", lab == "quad",
             lab == "tri", lab == "moving", lab == "quad_chain"]
    for w in range(len(lab) // 64):
        for k in kinds:
            assert k[64 * w:64 * w + 64].any(), w


# -------------------------------------------------------------------------- the dielectric
def _dielectric(c, a):
    m = _is(c, "diel_15", "diel_inv", "diel_24") & a["hit"]
    ri = np.select([c["label"][m] == "diel_15", c["label"][m] == "diel_inv"], [1.5, 1.0 / 1.5], 2.4)
    ri_eff, ud, cos, sin, raw = S.dielectric_terms(c["ray"][m, 3:6], a["n"][m], a["front"][m], ri)
    return m, ri_eff, ud, cos, sin, raw


def test_total_internal_reflection_is_met_within_ulps_on_both_sides():
    _, c, a = _mixed()
    m, ri_eff, ud, cos, sin, _ = _dielectric(c, a)
    val = ri_eff * sin
    near = np.abs(val - 1.0) <= 8 * ULP1
    front = a["front"][m]
    assert (near & (val > 1.0)).sum() >= 200 and (near & ~(val > 1.0)).sum() >= 200
    for side in (front, ~front):  # entering (ri 1/1.5) and leaving (1.5, 2.4)
        assert (near & side & (val > 1.0)).sum() >= 50 and (near & side & ~(val > 1.0)).sum() >= 50
    assert (val == 1.0).sum() >= 1  # the comparison's own edge
    # the oracle reflects exactly where this restatement says it cannot refract
    n = a["n"][m]
    refl = ud - n * (2.0 * S.dot3(ud, n))[:, None]
    tir = val > 1.0
    assert np.array_equal(a["dir"][m][tir], refl[tir])
    assert a["scatter"][m].all() and np.all(a["attenuation"][m] == 1.0)


def test_normal_and_grazing_incidence_are_met():
    _, c, a = _mixed()
    m, ri_eff, ud, cos, sin, raw = _dielectric(c, a)
    assert (raw > 1.0).sum() >= 1 and (raw == 1.0).sum() >= 1  # the min clamp matters, and its edge
    assert ((1.0 - cos) ** 5 > 0.999).sum() >= 20              # Schlick's x^5 near 1
    assert (cos < 1e-6).sum() >= 10


def test_reflectance_and_refract_kats_agree_with_the_bounce():
    _, c, a = _mixed()
    m, ri_eff, ud, cos, sin, _ = _dielectric(c, a)
    idx = np.flatnonzero(m)
    rng = np.random.default_rng(1)
    pick = rng.choice(len(idx), 400, replace=False)
    n_refr = n_refl = 0
    for j in pick:
        i = idx[j]
        r = oracle.wyrand(int(a["state_hit"][i]), 1)[0][0]
        cannot = ri_eff[j] * sin[j] > 1.0
        fresnel = oracle.reflectance(cos[j], ri_eff[j]) > r
        nn = a["n"][i]
        if cannot or fresnel:
            want = ud[j] - nn * (2.0 * (ud[j, 0] * nn[0] + ud[j, 1] * nn[1] + ud[j, 2] * nn[2]))
            n_refl += 1
        else:
            want = oracle.refract(ud[j], nn, ri_eff[j])
            n_refr += 1
        assert np.array_equal(want, a["dir"][i]), i
    assert n_refr >= 50 and n_refl >= 50
    assert np.array_equal(S.draws(a["state_hit"][idx], a["state"][idx]), np.ones(len(idx)))  # one draw, always


# ------------------------------------------------------------------------------- the metal
def test_metal_is_absorbed_and_scattered_and_its_rejection_loop_repeats():
    _, c, a = _mixed()
    m = _is(c, "metal_0", "metal_03", "metal_1") & a["hit"]
    assert (a["scatter"][m]).sum() >= 200 and (~a["scatter"][m]).sum() >= 200
    one = _is(c, "metal_1") & a["hit"]
    assert a["scatter"][one].sum() >= 100 and (~a["scatter"][one]).sum() >= 100  # either sign at fuzz 1
    assert a["scatter"][_is(c, "metal_0") & a["hit"]].all()
    d = S.draws(a["state_hit"][m], a["state"][m])
    assert (d % 3 == 0).all() and (d == 3).sum() >= 200 and (d > 3).sum() >= 200 and (d > 6).sum() >= 20
    assert np.all(a["emitted"][m] == 0.0) and np.all(a["dir"][m][~a["scatter"][m]] == 0.0)
    graze = m & (c["tag"] == "graze")
    ud = S.unit3(c["ray"][graze, 3:6])
    assert (np.abs(S.dot3(ud, a["n"][graze])) < 1e-3).sum() >= 50


# -------------------------------------------------------------------------- the Lambertian
def test_onb_axis_switch_is_met_at_its_edge_on_both_faces():
    _, c, a = _mixed()
    m = np.char.startswith(c["label"], "lamb") & a["hit"]
    w = S.unit3(a["n"][m])
    big = np.abs(w[:, 0]) > 0.9
    assert big.sum() >= 200 and (~big).sum() >= 200
    assert a["front"][m].sum() >= 200 and (~a["front"][m]).sum() >= 200
    ax = np.abs(w[:, 0])
    for v in (0.9, np.nextafter(0.9, 1.0), np.nextafter(0.9, 0.0), 1.0):
        for sign in (1.0, -1.0):
            for front in (True, False):
                assert ((w[:, 0] == sign * v) & (a["front"][m] == front)).sum() >= 1, (v, sign, front)
    assert (np.abs(ax - 0.9) <= 4 * 2.0 ** -53).sum() >= 400
    assert np.array_equal(S.draws(a["state_hit"][m], a["state"][m]), np.full(m.sum(), 2))


def test_onb_and_cosine_direction_kats_agree_with_the_bounce():
    _, c, a = _mixed()
    idx = np.flatnonzero(np.char.startswith(c["label"], "lamb") & a["hit"])
    rng = np.random.default_rng(2)
    for i in rng.choice(idx, 400, replace=False):
        r, _ = oracle.wyrand(int(a["state_hit"][i]), 2)
        x, y, z = oracle.random_cosine_direction(r[0], r[1])
        u, v, w = oracle.onb(a["n"][i])
        t = u * x + v * y + w * z  # ONB::transform (ONB.rs:25-27)
        assert np.array_equal(t / np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]), a["dir"][i]), i


# ------------------------------------------------------------------------------- textures
def test_every_texture_kind_and_both_checker_parities_are_hit():
    sc, c, a = _mixed()
    for lab in ("lamb_solid", "lamb_checker", "lamb_tree", "lamb_noise", "lamb_image", "light_solid", "light_image",
                "medium_solid", "medium_tex", "moving", "quad", "tri", "quad_chain"):
        assert (_is(c, lab) & a["hit"]).sum() >= 60, lab

    def count(lab, key, rgb):
        return np.all(a[key][_is(c, lab) & a["hit"]] == np.array(rgb), axis=1).sum()
    assert count("lamb_checker", "attenuation", (0.2, 0.3, 0.1)) >= 20
    assert count("lamb_checker", "attenuation", (0.9, 0.9, 0.9)) >= 20
    assert count("medium_tex", "attenuation", (0.9, 0.2, 0.2)) >= 20
    assert count("medium_tex", "attenuation", (0.2, 0.2, 0.9)) >= 20
    odd_outer, odd_inner = count("lamb_tree", "attenuation", (0.1, 0.8, 0.3)), count("lamb_tree", "attenuation", (0.9, 0.1, 0.2))
    m = _is(c, "lamb_tree") & a["hit"]
    assert odd_outer >= 20 and odd_inner >= 10 and a["image_texels"][m].sum() >= 10
    assert odd_outer + odd_inner + a["image_texels"][m].sum() == m.sum()
    assert a["noise_evals"][_is(c, "lamb_noise") & a["hit"]].all()
    assert np.all(a["emitted"][_is(c, "light_solid") & a["hit"]] == (4.0, 3.0, 2.0))
    assert not a["scatter"][_is(c, "light_solid", "light_image")].any()


def test_checker_kat_agrees_with_the_bounce():
    _, c, a = _mixed()
    idx = np.flatnonzero(_is(c, "lamb_checker") & a["hit"])
    for i in idx:
        even = oracle.checker_even(0.32, a["p"][i])
        assert np.array_equal(a["attenuation"][i], (0.2, 0.3, 0.1) if even else (0.9, 0.9, 0.9)), i


@pytest.mark.parametrize("name", ["mixed", "spheres_uv"])
def test_sphere_uv_reaches_the_poles_the_seam_and_every_texel(name):
    c, a = S.cases(name), S.answers(name)
    m = _is(c, "lamb_image", "light_image") & a["hit"]
    u, v = a["u"][m], a["v"][m]
    assert (u == 0.0).sum() >= 2 and (u == 1.0).sum() >= 2 and (v == 0.0).sum() >= 2 and (v == 1.0).sum() >= 2
    assert ((u > 0.0) & (u < 1e-3)).sum() >= 4 and ((u < 1.0) & (u > 1.0 - 1e-3)).sum() >= 4
    far = S.image_far(u, v, 5, 3)
    assert (~far).sum() >= 8  # on a texel boundary: the poles, the seam
    col = np.where(_is(c, "light_image")[m][:, None], a["emitted"][m], a["attenuation"][m])
    img = S._image_5x3().reshape(-1, 3) * (1.0 / 255.0)
    assert {tuple(x) for x in col[far]} == {tuple(x) for x in img}
    assert np.all(a["image_texels"][m] == 1)
    if name == "mixed":  # a sphere, a quad and a triangle under the same image: u, v of each kind
        for lab in ("quad", "tri"):
            k = _is(c, lab) & a["hit"]
            assert len({tuple(x) for x in a["attenuation"][k]}) >= 8, lab


@pytest.mark.parametrize("name", ["mixed", "spheres_uv", "deep"])
def test_image_texels_an_ulp_can_move_are_under_one_percent(name):
    """Of all the image texels a scene's cases reach through a sphere's u, v -- every object,
    every kind of case, the poles and the seam included -- at least 99% lie farther than 1e-9
    from a texel boundary in u W and (1 - v) H.  Closer, an ulp of acos / atan2 may choose the
    texel; the device test compares those colours only where the device's acos and atan2 return
    libm's bits, and the split form, which is given u and v, on all of them."""
    c, a = S.cases(name), S.answers(name)
    group = S.uv_texel_group(c, a)
    far = S.image_far(a["u"][group], a["v"][group], 5, 3)
    assert group.sum() >= 500 and far.mean() >= 0.99
    assert set(c["label"][group]) == {"mixed": {"lamb_image", "light_image", "lamb_tree"}, "spheres_uv": {"lamb_image"},
                                      "deep": {"chain1", "chain5", "chain6", "chain3_in_bvh_chain2"}}[name]


@pytest.mark.parametrize("name", ["sky_rgbe", "sky_f32"])
def test_sky_cases_sample_every_texel_away_from_its_edges(name):
    sc, c, a = S.scene(name), S.cases(name), S.answers(name)
    miss = ~a["hit"]
    uW, vH = S.sky_angles(c["ray"][miss, 3:6])
    far = S.sky_far(uW, vH)
    assert far.mean() >= 0.99  # (the share the device test compares)
    x = np.floor(np.maximum(uW, 0.0)).astype(np.int64) % S.SKY_W
    y = np.floor(np.maximum(vH, 0.0)).astype(np.int64) % S.SKY_H
    assert len(set(zip(x[far], y[far]))) == S.SKY_W * S.SKY_H
    tex = sc.extra["hdri"].astype(np.float64)
    assert np.array_equal(a["bg"][miss][far], tex[y[far], x[far]])  # HDRI::sample, restated
    assert np.all(a["hdri_texels"][miss] == 1) and (~far).sum() >= 1
    black = np.all(tex == 0.0, axis=2)
    assert black.sum() >= 4 and black[y[far], x[far]].sum() >= 4  # RGBE's e == 0
    if name == "sky_f32":
        assert np.all(tex[3, 5] == np.float32([0.1, 0.2, 0.3]).astype(np.float64)) and ((x[far] == 5) & (y[far] == 3)).any()


def test_media_draw_inside_the_hit_and_scatter_isotropically():
    _, c, a = _mixed()
    m = _is(c, "medium_solid", "medium_tex")
    before = S.draws(c["s0"][m], a["state_hit"][m])
    assert (before == 1).sum() >= 300 and set(before) <= {0, 1}  # ConstantMedium::hit's free-flight draw
    h = m & a["hit"]
    d = S.draws(a["state_hit"][h], a["state"][h])
    assert (d % 3 == 0).all() and (d > 3).sum() >= 50
    assert np.all(a["n"][h][:, 1:] == 0.0) and np.all(np.abs(a["n"][h][:, 0]) == 1.0)
    assert np.all(a["u"][h] == 0.0) and np.all(a["v"][h] == 0.0)


# ----------------------------------------------------------------------- kat_texture's cases
def test_texture_cases_reach_every_texel_parity_and_cast_edge():
    tex, u, v, p, what = S.texture_cases()
    col, img, noise = S.world("mixed").texture_value(tex, u, v, p)
    image = np.char.startswith(what, "image")
    assert np.all(img[image] == 1) and np.all(noise[what == "noise"] == 1)
    texels = S._image_5x3().reshape(-1, 3) * (1.0 / 255.0)
    assert {tuple(x) for x in col[image]} == {tuple(x) for x in texels}
    assert np.isnan(u[image]).sum() >= 7 and np.isnan(v[image]).sum() >= 7 and (u[image] == 1.0).sum() >= 7
    for k in range(6):  # u W on, and an ulp either side of, every integer
        assert {-1.0, 0.0, 1.0} <= set(np.sign(u[what == "image_u"] * 5.0 - k)), k
    for k in range(4):
        assert {-1.0, 0.0, 1.0} <= set(np.sign(v[what == "image_v"] * 3.0 - k)), k

    def count(w, rgb):
        return np.all(col[np.char.startswith(what, w)] == np.array(rgb), axis=1).sum()
    assert count("checker", (0.2, 0.3, 0.1)) >= 100 and count("checker", (0.9, 0.9, 0.9)) >= 100
    assert count("tree_", (0.1, 0.8, 0.3)) >= 100 and count("tree_", (0.9, 0.1, 0.2)) >= 50   # outer odd, inner odd
    assert img[np.char.startswith(what, "tree_")].sum() >= 50                                       # inner even
    assert count("tree_inner", (0.9, 0.1, 0.2)) >= 100 and img[np.char.startswith(what, "tree_inner")].sum() >= 100
    edge = np.char.endswith(what, "_edge")
    assert np.isnan(p[edge]).any() and np.isinf(p[edge]).any() and (np.abs(p[edge]) > 1e9).any()
    assert np.signbit(p[edge][p[edge] == 0.0]).any()
    # the wrapping i32 sum is reached: three saturated casts
    big = edge & np.all(np.abs(p) >= 2.0 ** 31 * 0.37, axis=1) & ~np.isnan(p).any(axis=1)
    assert big.sum() >= 20


def test_new_entries_restate_the_existing_ones():
    """oracle.World.texture_value against oracle.checker_even and oracle.noise_value."""
    tex, u, v, p, what = S.texture_cases()
    col, _, _ = S.world("mixed").texture_value(tex, u, v, p)
    for i in np.flatnonzero(np.char.startswith(what, "checker"))[:400]:
        even = oracle.checker_even(0.32, p[i])
        assert np.array_equal(col[i], (0.2, 0.3, 0.1) if even else (0.9, 0.9, 0.9)), i
    for i in np.flatnonzero(what == "noise")[:100]:
        assert col[i, 0] == oracle.noise_value(4.0, p[i]) and col[i, 0] == col[i, 1] == col[i, 2]
