"""The kernel lattice of the brute renderer (tests/kernel_matrix_ref.py), the parts that need no GPU: the enumeration; the ray classes
of every walk that tests/test_gpu_kernel_matrix.py compares against, asserted from the reference alone; that every axis of the lattice
engages in the reference (another lookup, a disc, another step form give another frame or other counters); the reference without a
disc pinned to step_scale_ref.brute -- schwarzschild_ref.compose_brute, over curvis_walk_ray, for the Schwarzschild kind --, every pixel and every
counter; and the conditions of the two edge scenes of the disc loop."""
import numpy as np
import pytest

import disc_ref as D
import kernel_matrix_ref as K
import oracle_lib as O
import step_scale_ref as SR

WALK_STEPS = ("fast", "scaled", "heun")        # the three step walks; strict shares fast's
BIG, SMALL = K.GRIDS[1], K.GRIDS[8]


def test_enumeration():
    cells = K.cells()
    assert len(cells) == 384 and len(set(cells)) == 384
    assert len(K.KINDS) == 4 and len(K.STEPS) == 4 and len(K.SUPERSAMPLES) == 4 and len(K.LOOKUPS) == 3 and len(K.PROJECTIONS) == 2
    assert len(K.inner_cells()) == 24 and {(k, s) + c for k in K.KINDS for s in K.STEPS for c in K.inner_cells()} == set(cells)
    relay = K.relay_cells()
    assert len(relay) == 96 and len(set(relay)) == 96 and set(relay) <= set(cells)
    # a cell is selected by its options: no two cells of a kind share them
    for kind in K.KINDS:
        opts = [tuple(sorted(K.cell_options(*c[1:]).items())) for c in cells if c[0] == kind]
        assert len(set(opts)) == 96
    # the grids: supersample 1, 2, 4 over one ragged fine grid, 8 over whole tiles; every frame has at least one pixel
    assert BIG[0] % 8 and BIG[1] % 8 and K.GRIDS[2] == K.GRIDS[4] == BIG and SMALL == (16, 8)
    assert [K.product_res(n) for n in K.SUPERSAMPLES] == [(20, 12), (10, 6), (5, 3), (2, 1)]
    assert set(K.STEP_WALKS[s] for s in WALK_STEPS) == set(K.STEP_WALKS.values()) and K.STEP_WALKS["strict"] == K.STEP_WALKS["fast"]


def test_scenes():
    for kind, name in (("ellis", "A"), ("interstellar", "B")):
        assert K.scene_parameters(kind) == D.SCENES[name][1:5] + (D.SCENES[name][6],) and D.SCENES[name][0] == kind
    _, _, _, disc = D.schwarzschild_scene()
    sc = K.scene("schwarzschild", D.SCHW_RES)       # disc_ref's scene moved (kernel_matrix_ref says why): the disc still starts at 6 M
    assert sc[1] is None and sc[5].l_in == disc.l_in and sc[5].l_out == K.SCHW_L_OUT and tuple(sc[3].pos) == K.SCHW_POS
    sc = K.cell_scene("flat", 4)
    assert (sc[3].res_x, sc[3].res_y) == BIG and (sc[4].resolution_width, sc[4].resolution_height) == (5, 3)


@pytest.mark.parametrize("projection", K.PROJECTIONS)
@pytest.mark.parametrize("step", WALK_STEPS)
@pytest.mark.parametrize("kind", K.KINDS)
def test_walks_hold_their_classes_and_every_axis_engages(kind, step, projection):
    for grid in (BIG, SMALL):
        for disc in (True, False):
            rays = K.walk(kind, step, projection, grid, disc)
            print(kind, step, projection, grid, "disc" if disc else "plain", D.classes(rays), D.counters(rays, 0))
            K.assert_walk_classes(rays, (kind, step, projection, grid, disc), disc)
            c = D.counters(rays, 0)
            assert c[0] == grid[0] * grid[1] == c[2] + c[3] + c[4] + c[6] and (c[6] > 0) == disc
            if kind == "schwarzschild":
                assert c[3] >= 8, "the hole's shadow is in the frame"
    nearest, bilinear, mipmap = (K.fine_frame(kind, step, projection, BIG, lookup, True) for lookup in K.LOOKUPS)
    assert (bilinear[0] != nearest[0]).any(), "the filter engages"
    assert (mipmap[0] != bilinear[0]).any(), "the pyramid engages"
    assert nearest[1][:5] == bilinear[1][:5] == mipmap[1][:5] and nearest[1][6] == bilinear[1][6] == mipmap[1][6]
    on_disc = K.walk(kind, step, projection, BIG, True)["code"] == D.DISC
    assert np.array_equal(bilinear[0][on_disc], nearest[0][on_disc]) and np.array_equal(mipmap[0][on_disc], nearest[0][on_disc]), "a disc ray keeps its texel"
    for lookup in K.LOOKUPS:
        with_disc, plain = K.fine_frame(kind, step, projection, BIG, lookup, True), K.fine_frame(kind, step, projection, BIG, lookup, False)
        assert (with_disc[0] != plain[0]).any() and with_disc[1] != plain[1] and plain[1][6] == 0, "the disc engages"
        for n in (2, 4):      # ... and still does behind the box average
            assert (K.cell_frame(kind, step, n, lookup, projection, True)[0] != K.cell_frame(kind, step, n, lookup, projection, False)[0]).any()
    if step != "fast":
        for disc in (True, False):
            assert K.walk(kind, step, projection, BIG, disc)["steps"].sum() != K.walk(kind, "fast", projection, BIG, disc)["steps"].sum(), "the step form changes the walk"
    assert K.walk(kind, "strict", projection, BIG, True) is K.walk(kind, "fast", projection, BIG, True)
    if projection != "perspective":
        assert (nearest[0] != K.fine_frame(kind, step, "perspective", BIG, "nearest", True)[0]).any(), "the projection engages"


@pytest.mark.parametrize("kind", K.EQUIRECTANGULAR_KINDS)
def test_equirectangular_walks_hold_their_classes(kind):
    rays = K.walk(kind, "fast", "equirectangular", BIG, True)
    print(kind, "equirectangular", D.classes(rays))
    K.assert_walk_classes(rays, (kind, "equirectangular"), True)
    assert (K.fine_frame(kind, "fast", "equirectangular", BIG, "nearest", True)[0] != K.fine_frame(kind, "fast", "fisheye", BIG, "nearest", True)[0]).any()


# ---- pins: without a disc the composition is the one the other suites trust ----------------------------------------------------------
PINS = {"ellis": ("scaled", 1, "fisheye"), "interstellar": ("fast", 2, "perspective"), "flat": ("scaled", 8, "fisheye")}


@pytest.mark.parametrize("kind", sorted(PINS))
def test_without_a_disc_a_cell_is_step_scale_refs_composition(kind):
    step, n, projection = PINS[kind]
    _, om, _, oc, _, _ = K.cell_scene(kind, n)
    S, integrator = K.STEP_WALKS[step]
    assert integrator == 0
    want = SR.brute(om, oc, SR.world_dirs(oc, K.PROJECTION_OPTION[projection]), *SR.oracle_skies(), K.CAP, K.R, K.DELTA, S)
    got = K.cell_frame(kind, step, n, "nearest", projection, False)
    assert np.array_equal(got[0], want[0] if n == 1 else SR.box_average(want[0], n))
    assert got[1][:6] == want[1] and got[1][6] == 0
    rays = K.walk(kind, step, projection, K.GRIDS[n], False)
    assert rays["x"].tobytes() == want[2]["x"].tobytes() and rays["p"].tobytes() == want[2]["p"].tobytes()
    assert np.array_equal(rays["steps"], want[2]["steps"]) and np.array_equal(rays["code"], want[2]["code"])


@pytest.mark.parametrize("step", ["fast", "scaled", "heun"])
def test_without_a_disc_a_schwarzschild_cell_is_schwarzschild_refs_composition(step):
    """the walk over curvis_update_relativistic_object in Python against curvis_walk_ray, the kernels' loop compiled for the host"""
    import schwarzschild_ref as SW
    _, _, pm, oc, _, _ = K.cell_scene("schwarzschild", 1)
    S, integrator = K.STEP_WALKS[step]
    want = SW.compose_brute(pm, oc, SR.world_dirs(oc, K.PROJECTION_OPTION["fisheye"]), *SR.oracle_skies(), K.CAP, K.R, K.DELTA, S, integrator)
    got = K.cell_frame("schwarzschild", step, 1, "nearest", "fisheye", False)
    assert np.array_equal(got[0], want[0])
    assert got[1][:6] == want[1] and got[1][6] == 0
    assert np.array_equal(K.walk("schwarzschild", step, "fisheye", BIG, False)["code"], want[2])


# ---- the edges of the disc loop ------------------------------------------------------------------------------------------------------
def test_euler_caps_beside_a_hit():
    """measured when the scene was chosen: the Euler walk's median disc step count is 59"""
    assert K.beside_caps("fast") == K.beside_caps("strict") == (59, 60)
    assert K.cap_conditions("fast", 60) == (3, 3) and K.capped_frame("fast", 60)[1] == (384, 22285, 0, 0, 313, 0, 71)
    assert K.cap_conditions("fast", 59) == (1, 3) and K.capped_frame("fast", 59)[1] == (384, 21972, 0, 0, 316, 0, 68)


@pytest.mark.parametrize("step", K.STEPS)
def test_caps_beside_a_hit(step):
    for cap in K.beside_caps(step):
        last, missed = K.cap_conditions(step, cap)
        cnt = K.capped_frame(step, cap)[1]
        print(step, "cap", cap, "disc rays with steps == cap - 1:", last, "disc rays of the full cap with steps == cap, capped here:", missed, cnt)
        assert last >= 1 and missed >= 1, (step, cap, last, missed)
        assert cnt[4] >= missed and cnt[6] >= last and cnt[0] == cnt[2] + cnt[3] + cnt[4] + cnt[6]
    for cap in K.LOW_CAPS:
        _, cnt, rays = K.capped_frame(step, cap)
        # nothing escapes in two steps; a ray found on the disc by the one plane test of cap 2 counts one step
        assert cnt[1] == cap * rays["code"].size - cnt[6] and cnt[4] + cnt[6] == cnt[0], (step, cap, cnt)
        if cap < 2:
            assert cnt[6] == 0, "no plane test before the second iteration"


@pytest.mark.parametrize("step", K.STEPS)
def test_camera_below_the_plane(step):
    """a plane test in the first iteration would end every ray on one texel; the reference makes none and the scene keeps its classes"""
    hit = K.first_iteration_hit()
    assert hit is not None and K.below_scene()[3].pos[2] > np.pi / 2
    _, cnt, rays = K.below_frame(step)
    print("below the plane", step, "a first-iteration plane test would hit texel", hit, "classes", D.classes(rays), cnt)
    D.assert_classes(rays, ("below the plane", step))
    assert rays["steps"][rays["code"] == D.DISC].min() >= 1
    assert len({tuple(t) for t in rays["texel"][rays["code"] == D.DISC].tolist()}) >= 8, "disc rays on many texels, not on one"


def test_hit_and_escape_in_one_ballot():
    _, cnt, rays = K.ballot_frame()
    pairs = K.ballot_pairs(rays)
    print("ballot scene: classes", D.classes(rays), "counters", cnt, "(tile, k):", pairs)
    assert len(pairs) >= 1
    D.assert_classes(rays, "ballot scene")
    assert D.classes(rays) == (174, 200, 10, 27, 0) and len(pairs) == 2, "measured when the scene was chosen"
