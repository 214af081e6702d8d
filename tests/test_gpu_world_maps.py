"""-m gpu: world maps (environments.register_world_map).  mmd_sdf_grid_windows is the clamped gather bit for bit and mmd_sdf_grid_lookup
its numpy fp32 restatement (tests/world_map_model.py); the resident world texture is the host definition and every robot's slice its host
crop; a one-tile world is the occupancy map of the same bitmap; an obstacle just outside a window acts through it; a round and an MPD call
on windows split free from colliding as the host crops do; environments.update_world_map rebuilds and recuts in place."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, guides, map_textures, synth      # noqa: E402
from oracle import mmd_oracle as O                               # noqa: E402
import cases                                                     # noqa: E402
import world_map_model as M                                      # noqa: E402
from cases import H, D                                           # noqa: E402

WORLD = "TestWorld"
T = 25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


@pytest.fixture(scope="module")
def world():
    """(bitmap, host texture) of the 640 x 520 test world, registered for the module: the texture is computed once and read-only."""
    occ = M.world_bitmap()
    E.register_world_map(WORLD, occ)
    tex = E.world_map_texture(WORLD)
    occ.setflags(write=False)
    tex.setflags(write=False)
    yield occ, tex
    E.unregister_world_map(WORLD)


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    tiles, worlds = set(E.registered_maps()), set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)
    for name in set(E.registered_maps()) - tiles:
        E.unregister_map(name)


def _gc():
    import gpu_common
    return gpu_common


def words(a):
    """the 32-bit words of a float32 array or tensor (or the words themselves), on the host"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype in (np.float32, np.uint32)
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_words(got, want, what):
    got, want = words(got), words(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        where = np.argwhere(bad)[:4]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {where.tolist()}: device "
                             f"{[hex(got[tuple(w)]) for w in where]} host {[hex(want[tuple(w)]) for w in where]}")


def raw_cut(world_words, origins, nx, ny):
    """mmd_sdf_grid_windows, twice into the same buffer: NaN guard rows behind the output stay untouched, and the second call gives the
    first one's bits.  world_words uint32 [wnx, wny, 4] -> uint32 [n, nx, ny, 4]"""
    wnx, wny = world_words.shape[:2]
    n = len(origins)
    world_d = torch.from_numpy(world_words.view(np.int32).copy()).cuda()
    org_d = torch.tensor(origins, dtype=torch.int32).reshape(n, 2).cuda()
    buf = torch.full((n * nx * ny + 64, 4), float("nan"), device="cuda")
    runs = []
    for _ in range(2):
        _lib.launch("mmd_sdf_grid_windows", buf, C.c_void_p(world_d.data_ptr()), wnx, wny, C.c_void_p(org_d.data_ptr()), n, nx, ny,
                    C.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[n * nx * ny:]).all()), "wrote behind the windows"
        runs.append(buf[:n * nx * ny].view(torch.int32).cpu().numpy().view(np.uint32).reshape(n, nx, ny, 4).copy())
    assert np.array_equal(runs[0], runs[1]), "a second call into the same buffer differs"
    return runs[0]


# ---- 1. the raw cut is the clamped gather, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (1, 1), (37, 45)])
def test_raw_cut_is_the_clamped_gather(shape):
    nx, ny = shape
    wnx, wny = 37, 45
    rng = np.random.Generator(np.random.PCG64(41))
    world = rng.integers(0, 1 << 32, (wnx, wny, 4), dtype=np.uint64).astype(np.uint32)              # any 32-bit pattern
    world[3, 4] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000]                                 # quiet and signalling NaNs with payloads, -0
    world[0, 0] = [0x80000000, 0xFF800001, 0x7FFFFFFF, 0x00000001]
    world[36, 44] = [0xFFFFFFFF, 0x80000000, 0x7F800000, 0xFF800000]
    assert np.isnan(world.view(np.float32)).sum() > 8
    i32 = np.iinfo(np.int32)
    fixed = [(0, 0), (wnx - nx, wny - ny), (0, 0), (3, 4), (wnx - nx, wny - ny), (-3, -2), (-nx, 2), (2, -ny - 9), (wnx, 5), (5, wny + 7),
             (wnx - 1, wny - 1), (i32.min, i32.max), (i32.max, i32.min), (i32.min, 0), (0, i32.max)]
    more = np.stack([rng.integers(-10, wnx + 10, 70), rng.integers(-10, wny + 10, 70)], 1).tolist()
    sets = {1: [fixed[3]], 3: [fixed[1], fixed[5], fixed[8]], 70: fixed + [tuple(o) for o in more[:70 - len(fixed)]]}
    for n, origins in sets.items():
        assert len(origins) == n
        assert_same_words(raw_cut(world, origins, nx, ny), M.gather_windows(world, origins, nx, ny), f"{nx} x {ny} windows, n = {n}")


def test_raw_cut_at_the_real_shape(world):
    occ, tex = world
    origins = [M.WINDOW_A, M.WINDOW_B, (240, 120), (0, 0), M.WINDOW_A]
    got = raw_cut(words(tex), origins, 400, 400)
    assert_same_words(got, M.gather_windows(words(tex), origins, 400, 400), "five 400 x 400 windows of the test world")
    assert_same_words(got, words(E.world_map_windows(WORLD, origins)), "the host crop")


# ---- 2. the raw lookup is its numpy fp32 restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [((-1.5, 0.25), (2.0, 1.75)), ((2.0, 0.25), (-1.5, 1.75))])
def test_raw_lookup_is_the_fp32_restatement(limits):
    f = np.float32
    nx, ny = 31, 33
    lo, hi = np.asarray(limits[0], f), np.asarray(limits[1], f)
    rng = np.random.Generator(np.random.PCG64(42))
    grid = rng.standard_normal((nx, ny, 4)).astype(f)
    # cell edges per axis and one ulp either side, paired with the other axis' edges in another order
    ex = np.minimum(lo[0], hi[0]) + np.arange(nx + 1, dtype=f) * (np.abs(hi[0] - lo[0]) / f(nx))
    ey = np.minimum(lo[1], hi[1]) + np.arange(ny + 1, dtype=f) * (np.abs(hi[1] - lo[1]) / f(ny))
    ex = np.concatenate([ex, np.nextafter(ex, f(-np.inf)), np.nextafter(ex, f(np.inf))]).astype(f)
    ey = np.concatenate([ey, np.nextafter(ey, f(-np.inf)), np.nextafter(ey, f(np.inf))]).astype(f)
    edges = np.stack([np.resize(ex, 128), np.resize(ey[::-1], 128)], 1)
    inside = np.stack([rng.uniform(-1.5, 2.0, 256), rng.uniform(0.25, 1.75, 256)], 1).astype(f)
    outside = np.asarray([(-1.6, 1.0), (2.1, 1.0), (0.0, 0.2), (0.0, 1.8), (-9.0, -9.0), (9.0, 9.0), (-9.0, 9.0), (9.0, -9.0), (1e30, 1.0),
                          (0.0, -1e30), (3.0e38, -3.0e38), (-3.0e38, 3.0e38)], f)
    odd = np.asarray([(np.inf, 1.0), (-np.inf, 1.0), (0.0, np.inf), (0.0, -np.inf), (np.nan, 1.0), (0.0, np.nan), (np.nan, np.nan),
                      (np.inf, np.nan)], f)
    pts = np.ascontiguousarray(np.concatenate([edges, inside, outside, odd]), f)
    want = M.lookup(grid, lo, hi, pts)
    assert np.isnan(want[-len(odd):]).all() and np.isfinite(want[:-len(odd)]).all()
    grid_d, pts_d = torch.from_numpy(grid).cuda(), torch.from_numpy(pts).cuda()
    out = torch.full((len(pts) + 16, 4), float("nan"), device="cuda")
    for _ in range(2):
        _lib.launch("mmd_sdf_grid_lookup", out, _lib.require_gpu(grid_d), nx, ny, (C.c_float * 2)(*lo.tolist()), (C.c_float * 2)(*hi.tolist()),
                    _lib.require_gpu(pts_d), len(pts), _lib.require_gpu(out))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isnan(got[len(pts):]).all(), "wrote behind the output"
        got = got[:len(pts)]
        assert np.isnan(got[-len(odd):]).all(), "a point with a non-finite coordinate gives four NaNs"
        assert_same_words(got[:-len(odd)], want[:-len(odd)], f"lookup on a 31 x 33 grid over {limits}")
    assert len(np.unique(want[:128, 0])) > 16                       # the edge points land in many texels


# ---- 3. resident storage ------------------------------------------------------------------------------------------------------------------------
def _robots_across_the_shared_box():
    """4 robots in the two overlapping test windows, two each, whose straight lines cross the box both windows see (global (+-0.1, +-0.3))"""
    lo = np.asarray(E.world_map_limits(WORLD)[0])
    off_a, off_b = (np.float32(lo + 1.0 + 0.005 * np.asarray(w)) for w in (M.WINDOW_A, M.WINDOW_B))
    starts = np.float32([(-0.45, -0.1), (-0.4, 0.45), (0.45, 0.1), (0.4, -0.45)])
    goals = np.float32([(0.3, 0.1), (0.3, -0.45), (-0.3, -0.1), (-0.3, 0.45)])
    return starts, goals, np.stack([off_a, off_a, off_b, off_b]).astype(np.float32)


def test_resident_world_texture_and_robot_slices(world):
    from mmd_amd.world import WorldRobotSampler
    occ, tex = world
    wtex = guides.device_world_texture(WORLD, "cuda")
    assert wtex is guides.device_world_texture(WORLD, torch.device("cuda", 0)) and tuple(wtex.shape) == M.SHAPE + (4,)
    assert_same_words(wtex, tex, "the resident world texture")
    lo = np.asarray(E.world_map_limits(WORLD)[0])
    wanted = [M.WINDOW_A, (20, 40), M.WINDOW_B, M.WINDOW_B, (60, 120)]                         # two robots share an offset
    offsets = np.float32([lo + 1.0 + 0.005 * np.asarray(w) for w in wanted])
    origins = E.world_map_window_origins(WORLD, offsets)
    assert origins.tolist() == [list(w) for w in wanted]
    starts, goals = offsets + np.float32([-0.8, -0.8]), offsets + np.float32([0.8, -0.7])
    s = WorldRobotSampler(_gc().hip_model(T), starts, goals, offsets, env_id=WORLD, n_samples=4)
    assert s.guide._grids.shape == (4, 1, 400, 400, 4) and s.guide.desc().n_grids == 1 and s.guide.desc().n_maps == 4
    crops = E.world_map_windows(WORLD, origins)
    robot_map = s.guide._robot_map.cpu().tolist()
    assert robot_map[2] == robot_map[3] and len(set(robot_map)) == 4
    for r in range(5):
        assert_same_words(s.guide._grids[robot_map[r], 0], crops[r], f"robot {r}'s slice")
    # the texel of a point, read off the resident texture
    pts = np.random.Generator(np.random.PCG64(43)).uniform(-1.7, 1.7, (4096, 2)).astype(np.float32)
    pts[7] = [np.nan, 0.0]
    got = E.world_map_sdf(torch.from_numpy(pts), WORLD, device="cuda")
    assert got.is_cuda and got.shape == (4096,) and bool(torch.isnan(got[7]))
    assert_same_words(got, E.world_map_sdf(pts, WORLD).numpy(), "world_map_sdf on the device")


# ---- 4. a one-tile world is the occupancy map ----------------------------------------------------------------------------------------------------
def test_one_tile_world_is_the_occupancy_map(registry):
    import occupancy_model
    from mmd_amd.world import WorldRobotSampler
    occ = occupancy_model.test_occupancy()
    E.register_occupancy_map("Floor", occ)
    E.register_world_map("OneTile", occ, origin=(-1.0, -1.0))
    starts, goals = synth.start_goal_circle(4, 0.45)
    zero = np.zeros((4, 2), np.float32)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    out = []
    for env_id in ("OneTile", "Floor"):
        s = WorldRobotSampler(_gc().hip_model(T), starts, goals, zero, env_id=env_id, n_samples=4)
        assert s.guide.desc().n_grids == 1 and s.guide.desc().n_maps == 1
        out.append(s.plan_round(paths, seed=5) + (s.guide._grids,))
    assert out[0][2].data_ptr() != out[1][2].data_ptr()
    assert_same_words(out[0][2], out[1][2], "the window of the one-tile world and the occupancy map's texture")
    assert out[0][0].shape == (16, H, D) and torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 5. the world acts through the window ----------------------------------------------------------------------------------------------------------
def _grid_params(tex, cutoff=0.05):
    tex = torch.from_numpy(np.ascontiguousarray(tex))
    return O.GuideParams(norm_mins=cases.MINS, norm_maxs=cases.MAXS, sdf_grids=[(tex[..., 0].contiguous(), tex[..., 1:3].contiguous())],
                         cutoff_margin=cutoff)


def test_an_obstacle_outside_the_window_acts_through_it(world):
    """One guide evaluation on window A, whose lower border lies 5 cells above the bar outside it, against the oracle on the host crop:
    max abs < 2e-6, the bound of tests/test_gpu_occupancy_maps.py's single-evaluation test.  Three rows run along that border within the
    guide's margin (0.105 = 21 cells) of the bar; against the oracle on the transform of the CROPPED bitmap, which does not know the bar,
    the same evaluation differs by more than 1e-3."""
    occ, tex = world
    i0, j0 = M.WINDOW_A
    name = E.world_window_name(WORLD, M.WINDOW_A)
    crop = E.world_map_windows(WORLD, [M.WINDOW_A])[0]
    own = E.occupancy_sdf_texture(occ[i0:i0 + 400, j0:j0 + 400])
    x = torch.from_numpy(synth.synth_noise(61, (8, H, D))) * 0.6
    w = torch.linspace(0, 1, H)
    for r, y in enumerate((-0.97, -0.94, -0.91)):                  # local x over the bar's cells 100 .. 140 and a little beyond, 6 to 18 cells up
        x[r, :, 0], x[r, :, 1], x[r, :, 2:] = -0.52 + 0.24 * w, y, 0.0
    guide = _gc().hip_guide(name, [[]])
    assert guide.desc().n_grids == 1
    assert_same_words(guide._grids[0, 0], crop, "the resident window")
    got = guide.forward(x.cuda()).cpu()
    ref = O.guide_grad(x, _grid_params(crop), [], clip_mode="always")
    err = float((got - ref).abs().max())
    other = float((got - O.guide_grad(x, _grid_params(own), [], clip_mode="always")).abs().max())
    print(f"one guide evaluation on a window of the test world: max abs {err:.3e} against the crop, {other:.3e} against the cropped bitmap's transform")
    assert err < 2e-6
    assert other > 1e-3


# ---- 6. a round in a world ------------------------------------------------------------------------------------------------------------------------
def test_round_and_mpd_call_in_a_world(world):
    from mmd_amd import postprocess as post
    from mmd_amd.planners import MPD
    from mmd_amd.world import WorldRobotSampler
    occ, tex = world
    starts, goals, offsets = _robots_across_the_shared_box()
    origins = E.world_map_window_origins(WORLD, offsets)
    assert origins.tolist() == [list(M.WINDOW_A)] * 2 + [list(M.WINDOW_B)] * 2
    crops = E.world_map_windows(WORLD, origins)
    s = WorldRobotSampler(_gc().hip_model(T), starts, goals, offsets, env_id=WORLD, n_samples=4)
    assert s.guide._grids.shape[0] == 2
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    trajs, best = s.plan_round(paths, seed=5)
    assert trajs.shape == (16, H, D) and torch.isfinite(trajs).all() and best.shape == (4, H, 2) and torch.isfinite(best).all()
    t = s.unnormalize(trajs).contiguous()                          # every robot in its own frame: its window's
    free = np.concatenate([M.host_free_mask(crops[r], t[4 * r:4 * r + 4].cpu().numpy()) for r in range(4)])
    assert np.array_equal(post.postprocess_batch(s.guide, t, n_robots=4, smooth=False).free_mask.cpu().numpy().astype(bool), free)
    assert s.last_n_free.cpu().tolist() == free.reshape(4, 4).sum(1).tolist()
    # the same straight line in every robot's frame: through the shared box in window A's frame, clear of everything in window B's
    line = np.zeros((16, H, 4), np.float32)
    line[:, :, 0] = np.linspace(0.3, 0.9, H, dtype=np.float32)
    want = np.concatenate([M.host_free_mask(crops[r], line[4 * r:4 * r + 4]) for r in range(4)])
    assert want.tolist() == [False] * 8 + [True] * 8
    assert post.postprocess_batch(s.guide, torch.from_numpy(line).cuda(), n_robots=4, smooth=False).free_mask.cpu().numpy().astype(bool).tolist() == want.tolist()
    # one MPD call on a window's map name
    name = E.world_window_name(WORLD, offsets[0])
    start, goal = torch.from_numpy(starts[0] - offsets[0]), torch.from_numpy(goals[0] - offsets[0])
    p = MPD(model_id="EnvHighways2D-RobotPlanarDisk", env_id=name, planner_alg="mmd", start_state_pos=start, goal_state_pos=goal, device="cuda",
            seed=23, n_samples=8, model_state_dict=synth.synth_unet_state_dict(0), model_args=dict(n_diffusion_steps=T), trained_models_dir="")
    assert p.env_id == name
    res = p(start, goal)
    assert res.trajs_final.shape == (8, H, D) and torch.isfinite(res.trajs_final).all() and torch.isfinite(res.trajs_iters).all()
    free = M.host_free_mask(crops[0], res.trajs_iters[-1].cpu().numpy())      # the split is taken on the un-smoothed final samples
    assert sorted(res.trajs_final_free_idxs.view(-1).tolist()) == np.flatnonzero(free).tolist()
    assert sorted(res.trajs_final_coll_idxs.view(-1).tolist()) == np.flatnonzero(~free).tolist()


# ---- 7. update_world_map ------------------------------------------------------------------------------------------------------------------------------
def test_update_world_map_rebuilds_and_recuts_in_place(registry):
    """N_TEXTURE_BUILDS' rule: 1 per texture a library call writes whole -- a world texture built from its bitmap, and each window slice
    of a cut."""
    from mmd_amd.world import WorldRobotSampler
    occ_a = np.zeros((400, 520), np.uint8)
    occ_a[150:260, 170:230] = 1
    occ_b = np.ascontiguousarray(M.world_bitmap()[:400])
    E.register_world_map("Moving", occ_a)
    lo = np.asarray(E.world_map_limits("Moving")[0])
    offsets = np.float32([lo + 1.0, lo + 1.0 + (0.0, 0.6), lo + 1.0])                          # origin cells (0, 0), (0, 120), (0, 0)
    starts, goals = offsets + np.float32([-0.8, -0.8]), offsets + np.float32([0.8, -0.7])
    names = [E.world_window_name("Moving", o) for o in offsets]
    assert names[0] == names[2] == "Moving@0,0" and names[1] == "Moving@0,120"
    uploads, builds = map_textures.N_TEXTURE_UPLOADS, map_textures.N_TEXTURE_BUILDS
    s = WorldRobotSampler(_gc().hip_model(T), starts, goals, offsets, env_id="Moving", n_samples=4)
    assert map_textures.N_TEXTURE_BUILDS == builds + 1 + 2 and map_textures.N_TEXTURE_UPLOADS == uploads     # the world texture, two window slices
    mixed = _gc().hip_guide("EnvEmpty2D", [[], []], n_robots=2, robot_env_ids=["EnvConveyor2D", names[1]])
    assert map_textures.N_TEXTURE_BUILDS == builds + 4 and map_textures.N_TEXTURE_UPLOADS == uploads + 1     # one more slice cut; Conveyor is an upload
    live = _gc().hip_guide(names[0], [[]])
    assert map_textures.N_TEXTURE_BUILDS == builds + 5
    assert _gc().hip_guide(names[0], [[]])._grids is live._grids and map_textures.N_TEXTURE_BUILDS == builds + 5      # shared, not cut again
    wtex = guides.device_world_texture("Moving", "cuda")
    assert map_textures.N_TEXTURE_BUILDS == builds + 5                                                 # resident already
    ptrs = (wtex.data_ptr(), s.guide._grids.data_ptr(), mixed._grids.data_ptr(), live._grids.data_ptr())
    conveyor = E.sdf_grid_texture("EnvConveyor2D")
    assert_same_words(mixed._grids[0, 0], conveyor, "the shipped slice")
    x = torch.from_numpy(synth.synth_noise(95, (4, H, D))) * 0.6
    hard = torch.zeros(1, 2, D, device="cuda")
    before = live.guide_steps(x.clone().cuda(), hard, 0, 5)

    builds = map_textures.N_TEXTURE_BUILDS
    E.update_world_map("Moving", occ_b)
    assert (wtex.data_ptr(), s.guide._grids.data_ptr(), mixed._grids.data_ptr(), live._grids.data_ptr()) == ptrs
    assert guides.device_world_texture("Moving", "cuda") is wtex
    assert map_textures.N_TEXTURE_BUILDS == builds + 1 + 2 + 1 + 1 and map_textures.N_TEXTURE_UPLOADS == uploads + 1      # the world; 2, 1 and 1 slices
    assert_same_words(wtex, E.world_map_texture("Moving"), "the world texture after the update")
    crops = E.world_map_windows("Moving", [(0, 0), (0, 120)])
    assert s.guide._robot_map.cpu().tolist() == [0, 1, 0]
    assert_same_words(s.guide._grids[:, 0], crops, "the sampler's slices after the update")
    assert_same_words(mixed._grids[1, 0], crops[1], "the mixed guide's window after the update")
    assert_same_words(mixed._grids[0, 0], conveyor, "the shipped slice is untouched")
    assert_same_words(live._grids[0, 0], crops[0], "the live guide's window after the update")
    E.register_world_map("Fresh", occ_b)
    fresh = _gc().hip_guide(E.world_window_name("Fresh", (0, 0)), [[]])
    after = live.guide_steps(x.clone().cuda(), hard, 0, 5)
    assert torch.equal(after, fresh.guide_steps(x.clone().cuda(), hard, 0, 5)) and not torch.equal(after, before)
    E.unregister_world_map("Moving")
    assert not any(k[0] == "Moving" for k in map_textures._WORLD_TEXTURES) and not any("Moving@" in m for k in map_textures._TEXTURES for m in k[0])
