"""-m gpu: occupancy maps (environments.register_occupancy_map).  The texture mmd_sdf_grid_from_occupancy builds on the device is the
host definition (environments.occupancy_sdf_texture; tests/test_occupancy_maps_host.py holds it to the brute force and to scipy) bit for
bit, and everything that reads the resident texture -- guide, samplers, planners, post-processing, per-robot maps -- runs on such a map
as on a shipped one.  environments.update_occupancy_map rebuilds the resident texture in place."""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, map_textures, synth      # noqa: E402
from oracle import mmd_oracle as O                               # noqa: E402
import cases                                                     # noqa: E402
import occupancy_model as M                                      # noqa: E402
from cases import H, D                                           # noqa: E402

SMALL = M.small_grids()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    before = set(E.registered_maps())
    yield
    for name in set(E.registered_maps()) - before:
        E.unregister_map(name)


@pytest.fixture(scope="module")
def test_map():
    """(bitmap, host texture) of the test map, computed once and read-only."""
    occ = M.test_occupancy()
    tex = E.occupancy_sdf_texture(occ)
    occ.setflags(write=False)
    tex.setflags(write=False)
    return occ, tex


def _gc():
    import gpu_common
    return gpu_common


def assert_same_bits(dev, host, what, occ=None, cell=None):
    """Every fp32 word the same, the sign of a zero included.  On a mismatch with occ given: whether the numpy restatement of the
    kernels' operation sequence agrees with the definition (then the device arithmetic differs from numpy's, not the algorithm)."""
    dev = dev.cpu().numpy()
    host = np.asarray(host)
    assert dev.shape == host.shape and dev.dtype == host.dtype == np.float32, (what, dev.shape, host.shape)
    bad = dev.view(np.uint32) != host.view(np.uint32)
    if bad.any():
        note = ""
        if occ is not None:
            note = f"; numpy restatement == definition: {np.array_equal(M.kernel_texture(occ, cell).view(np.uint32), host.view(np.uint32))}"
        where = np.argwhere(bad)[:4]
        raise AssertionError(f"{what}: {int(bad.any(-1).sum())} of {bad[..., 0].size} cells differ, first at {where.tolist()}: device "
                             f"{[dev[tuple(w[:2])].tolist() for w in where[:2]]} host {[host[tuple(w[:2])].tolist() for w in where[:2]]}{note}")


GUARD = 0xA5


def raw_device_grid(occ, cell):
    """mmd_sdf_grid_from_occupancy on any grid, twice into the same buffers: NaN guard cells behind the grid and guard bytes behind the
    workspace stay untouched, and the second call gives the first one's bits."""
    nx, ny = occ.shape
    lib = _lib.load()
    n_work = int(lib.mmd_sdf_grid_occupancy_work_bytes(nx, ny))
    assert n_work == 4 * nx * ny
    buf = torch.full((nx * ny + 64, 4), float("nan"), device="cuda")
    work = torch.full((n_work + 256,), GUARD, dtype=torch.uint8, device="cuda")
    occ_d = torch.from_numpy(np.ascontiguousarray(occ, dtype=np.uint8) * np.uint8(255)).cuda()         # non-zero = occupied
    runs = []
    for _ in range(2):
        _lib.launch("mmd_sdf_grid_from_occupancy", buf, C.c_void_p(occ_d.data_ptr()), nx, ny, float(cell), C.c_void_p(buf.data_ptr()),
                    C.c_void_p(work.data_ptr()), n_work)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[nx * ny:]).all()), "wrote behind the grid"
        assert bool((work[n_work:] == GUARD).all()), "wrote behind the workspace"
        runs.append(buf[:nx * ny].view(nx, ny, 4).clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "a second call into the same buffers differs"
    return runs[0]


@pytest.mark.parametrize("case", list(SMALL))
def test_raw_entry_is_the_definition_small_shapes(case):
    occ, cell = SMALL[case]
    host = E.occupancy_sdf_texture(occ, cell)
    assert_same_bits(raw_device_grid(occ, cell), host, case, occ, cell)
    if case == "31x33 coarse":
        assert ((host[..., 0] == 1) & (occ == 0)).any()                          # the cap acts on this grid


def test_raw_entry_is_the_definition_on_the_test_map(test_map):
    occ, tex = test_map
    assert_same_bits(raw_device_grid(occ, E.SDF_CELL_SIZE), tex, "test map", occ, E.SDF_CELL_SIZE)


@pytest.mark.parametrize("fill", [0, 1])
def test_raw_entry_all_free_and_all_occupied(fill):
    """No site anywhere: decided on the device, (1, 0, 0, 0) or (-1, 0, 0, 0) in every cell."""
    for shape in ((400, 400), (3, 130)):
        occ = np.full(shape, fill, np.uint8)
        assert_same_bits(raw_device_grid(occ, 0.005), E.occupancy_sdf_texture(occ), f"all {fill} {shape}")


def test_device_occupancy_sdf_grid_and_out(test_map):
    occ, tex = test_map
    dev = E.device_occupancy_sdf_grid(occ, "cuda")
    assert tuple(dev.shape) == (400, 400, 4) and dev.dtype == torch.float32 and dev.is_cuda
    assert_same_bits(dev, tex, "device_occupancy_sdf_grid")
    flipped = np.ascontiguousarray(occ[:, ::-1])
    again = E.device_occupancy_sdf_grid(torch.from_numpy(flipped).cuda().bool(), "cuda", out=dev)        # a device tensor, in place
    assert again.data_ptr() == dev.data_ptr()
    assert_same_bits(again, E.occupancy_sdf_texture(flipped), "out=, from a device tensor", flipped, E.SDF_CELL_SIZE)
    with pytest.raises(ValueError):
        E.device_occupancy_sdf_grid(occ, "cuda", out=torch.empty(400, 400, 3, device="cuda"))
    with pytest.raises(ValueError):
        E.device_occupancy_sdf_grid(occ[:200], "cuda")
    with pytest.raises(ValueError):
        E.device_occupancy_sdf_grid(torch.zeros(200, 400, device="cuda"), "cuda")


def _grid_params(name, cutoff=0.05):
    """GuideParams whose one SDF grid is the HOST texture of a registered map."""
    tex = torch.from_numpy(E.sdf_grid_texture(name))
    return O.GuideParams(norm_mins=cases.MINS, norm_maxs=cases.MAXS, sdf_grids=[(tex[..., 0].contiguous(), tex[..., 1:3].contiguous())],
                         cutoff_margin=cutoff)


def test_guide_single_evaluation_on_an_occupancy_map_vs_oracle(registry, test_map):
    """One guide evaluation on the registered test map against the oracle on the host texture: the inputs and the bound of
    tests/test_gpu_custom_maps.py's and tests/test_gpu_parity.py's single-evaluation checks, max abs < 2e-6."""
    E.register_occupancy_map("Floor", test_map[0])
    x = torch.from_numpy(synth.synth_noise(60, (8, H, D))) * 0.6
    guide = _gc().hip_guide("Floor", [[]])
    assert guide.desc().n_grids == 1
    assert_same_bits(guide._grids[0, 0], test_map[1], "the resident texture")
    got = guide.forward(x.cuda()).cpu()
    ref = O.guide_grad(x, _grid_params("Floor"), [], clip_mode="always")
    err = float((got - ref).abs().max())
    print(f"one guide evaluation on the occupancy test map: max abs {err:.3e}")
    assert err < 2e-6
    assert float((ref - O.guide_grad(x, cases.guide_params("EnvEmpty2D"), [], clip_mode="always")).abs().max()) > 1e-3      # the map acts


def test_guide_20_steps_on_an_occupancy_map_teacher_forced(registry, test_map):
    """20 chained guide iterations on the registered test map with the inputs and constraints of test_guide_20_steps_vs_oracle
    (tests/test_gpu_parity.py), every iteration against the oracle on the host texture restarted from the kernel's state before it:
    max abs < 2e-6 per iteration, the bound of tests/test_gpu_custom_maps.py's teacher-forced test."""
    E.register_occupancy_map("Floor", test_map[0])
    starts, goals, soft, hard = cases.highways_case()
    gp = _grid_params("Floor")
    hc = cases.hard_conds_for(starts[3], goals[3])
    x = O.apply_hard_conditioning(torch.from_numpy(synth.synth_noise(50, (8, H, D))) * 0.5, hc)
    guide = _gc().hip_guide("Floor", [[soft, hard]])
    y = x.clone().cuda()
    chain = torch.empty((20,) + tuple(y.shape), device="cuda")
    guide.guide_steps(y, torch.stack([hc[0], hc[H - 1]])[None].cuda().contiguous(), _lib.HARD_ROWS_START_GOAL, 20, chain=chain)
    chain = chain.cpu()
    assert torch.equal(chain[-1], y.cpu())
    empty = cases.guide_params("EnvEmpty2D")
    prev, worst, moved = x, 0.0, 0.0
    for k in range(20):
        step = O.guide_grad(prev, gp, [soft, hard], clip_mode="always")
        moved = max(moved, float((step - O.guide_grad(prev, empty, [soft, hard], clip_mode="always")).abs().max()))
        worst = max(worst, float((O.apply_hard_conditioning(prev + step, hc) - chain[k]).abs().max()))
        prev = chain[k]
    print(f"20 guide steps on the occupancy test map, teacher-forced: worst max abs {worst:.3e}")
    assert worst < 2e-6
    assert moved > 1e-3


def _nearest_cell_collides(tex, px, py, margin):
    """PlanningTask.compute_collision on the grid (grid_map_sdf.py:84-99, tasks.py:204-232) in numpy fp32: nearest cell of the host
    texture or a workspace boundary (1.08 x the limits, tasks.py:81-83) nearer than margin."""
    f = np.float32
    n = f(tex.shape[0])
    ix = np.clip(np.floor((px - f(-1)) / f(2) * n).astype(np.int64), 0, tex.shape[0] - 1)
    iy = np.clip(np.floor((py - f(-1)) / f(2) * n).astype(np.int64), 0, tex.shape[1] - 1)
    lo, hi = f(-1) * f(1.08), f(1) * f(1.08)
    return (tex[ix, iy, 0] < margin) | (px - lo < margin) | (py - lo < margin) | (hi - px < margin) | (hi - py < margin)


def _host_free_mask(tex, trajs):
    """postprocess_batch's free flag of un-normalised trajectories [n, H, 4] by the host texture: no interpolated point (5 per segment)
    collides at the robot radius and every support point is inside the joint limits."""
    from mmd_amd import postprocess as post
    f = np.float32
    trajs = np.asarray(trajs, f)
    alpha = post.interpolation_alphas(5)
    px = trajs[:, :-1, None, 0] * alpha + trajs[:, 1:, None, 0] * (f(1) - alpha)
    py = trajs[:, :-1, None, 1] * alpha + trajs[:, 1:, None, 1] * (f(1) - alpha)
    coll = _nearest_cell_collides(tex, px, py, f(post.ROBOT_RADIUS)).reshape(len(trajs), -1)
    q_min, q_max = np.asarray(post.Q_MIN, f), np.asarray(post.Q_MAX, f)
    inside = ((trajs[..., :2] >= q_min) & (trajs[..., :2] <= q_max)).all((1, 2))
    return coll, ~coll.any(1) & inside


def test_postprocess_and_compute_collision_are_the_host_textures_nearest_cell(registry, test_map):
    from mmd_amd import postprocess as post
    occ, tex = test_map
    E.register_occupancy_map("Floor", occ)
    guide = _gc().hip_guide("Floor", [[]])
    f = np.float32
    # straight lines through the boxes, the bar, the disc, the thin wall and its one-cell gap; beside a box's edge (surface + radius -+ a
    # cell or two); and clear of everything (between the boxes, above the disc, inside the ring's pocket)
    ends = [((-0.9, -0.6), (0.9, -0.6)), ((-0.05, -0.9), (-0.05, 0.9)), ((-0.9, 0.0), (0.2, 0.002)), ((0.1, 0.4), (0.9, 0.41)),
            ((-0.5125, -0.2), (-0.5125, 0.12)), ((-0.85, -0.4525), (-0.35, -0.4525)), ((-0.85, -0.4425), (-0.35, -0.4425)),
            ((-0.85, -0.4475), (-0.35, -0.4475)), ((-0.85, -0.45), (-0.35, -0.445)), ((-0.7, -0.93), (0.1, -0.93)), ((0.3, 0.8), (0.8, 0.85)),
            ((-0.3, -0.9), (0.15, -0.3)), ((-0.64, 0.345), (-0.56, 0.345)), ((-0.68, 0.3), (-0.52, 0.3)), ((0.3, 0.05), (0.85, 0.1)),
            ((0.85, 0.85), (0.95, 0.95))]
    w = np.linspace(0, 1, H, dtype=np.float32)[:, None]
    trajs = np.zeros((len(ends), H, 4), np.float32)
    for k, (a, b) in enumerate(ends):
        trajs[k, :, :2] = np.asarray(a, f) * (f(1) - w) + np.asarray(b, f) * w
    want, free = _host_free_mask(tex, trajs)
    assert free.any() and not free.all() and want[0].any() and want[4].any() and want[5].any() and free[6] and free[9] and free[12]
    r = post.postprocess_batch(guide, torch.from_numpy(trajs).cuda(), num_interpolation=5, smooth=False, want_waypoints=True)
    assert np.array_equal(r.waypoint_collisions.cpu().numpy().astype(bool), want)
    assert np.array_equal(r.free_mask.cpu().numpy().astype(bool), free)
    pts = np.random.Generator(np.random.PCG64(93)).uniform(-1, 1, (4096, 2)).astype(np.float32)
    hit = post.compute_collision(torch.from_numpy(pts).cuda(), guide, margin=0.05).cpu().numpy()
    assert np.array_equal(hit, _nearest_cell_collides(tex, pts[:, 0], pts[:, 1], f(0.05))) and hit.any() and not hit.all()


def test_per_robot_maps_mix_shipped_primitive_and_occupancy(registry, test_map):
    """robot_env_ids = a shipped, a primitive and an occupancy map in one guide: each robot's rows are its single-map guide's."""
    E.register_occupancy_map("Floor", test_map[0])
    E.register_map("Prims", [(0.0, 0.0, 0.6, 0.3), (-0.5, 0.6, 0.2, 0.5)], [(0.5, 0.5, 0.2)])
    B = 4
    x = torch.from_numpy(synth.synth_noise(94, (3 * B, H, D))) * 0.6
    hard = torch.zeros(3, 2, D, device="cuda")
    env_ids = ["EnvHighways2D", "Prims", "Floor"]
    mixed = _gc().hip_guide("EnvEmpty2D", [[], [], []], n_robots=3, robot_env_ids=env_ids)
    assert mixed._grids.shape[0] == 3 and mixed.desc().n_grids == 1
    y = x.clone().cuda()
    mixed.guide_steps(y, hard, 0, 5)
    for r, env_id in enumerate(env_ids):
        z = x[r * B:(r + 1) * B].clone().cuda()
        _gc().hip_guide(env_id, [[]]).guide_steps(z, hard[:1].contiguous(), 0, 5)
        assert torch.equal(y[r * B:(r + 1) * B], z), (r, env_id)
    x2 = x[2 * B:].clone().cuda()
    _gc().hip_guide("Prims", [[]]).guide_steps(x2, hard[:1].contiguous(), 0, 5)
    assert not torch.equal(x2, y[2 * B:])                                    # the maps act differently on the same rows


def test_update_occupancy_map_rebuilds_the_resident_texture_in_place(registry, test_map):
    occ_b, host_b = test_map
    occ_a = np.zeros((400, 400), np.uint8)
    occ_a[150:260, 170:230] = 1
    occ_c = np.ascontiguousarray(occ_b[::-1, ::-1])
    E.register_occupancy_map("Moving", occ_a)
    uploads, builds = map_textures.N_TEXTURE_UPLOADS, map_textures.N_TEXTURE_BUILDS
    old = _gc().hip_guide("Moving", [[]])
    both = _gc().hip_guide("EnvEmpty2D", [[], []], n_robots=2, robot_env_ids=["EnvConveyor2D", "Moving"])
    assert map_textures.N_TEXTURE_BUILDS == builds + 2 and map_textures.N_TEXTURE_UPLOADS == uploads + 1     # (the Conveyor slice is an upload)
    assert _gc().hip_guide("Moving", [[]])._grids is old._grids and map_textures.N_TEXTURE_BUILDS == builds + 2      # shared, not rebuilt
    assert_same_bits(old._grids[0, 0], E.sdf_grid_texture("Moving"), "before the update")
    x = torch.from_numpy(synth.synth_noise(95, (4, H, D))) * 0.6
    hard = torch.zeros(1, 2, D, device="cuda")
    before = x.clone().cuda()
    old.guide_steps(before, hard, 0, 5)
    ptrs = (old._grids.data_ptr(), both._grids.data_ptr())
    conveyor = E.sdf_grid_texture("EnvConveyor2D")

    def updated(new, host, what):
        uploads, builds = map_textures.N_TEXTURE_UPLOADS, map_textures.N_TEXTURE_BUILDS
        E.update_occupancy_map("Moving", new)
        assert (old._grids.data_ptr(), both._grids.data_ptr()) == ptrs
        assert map_textures.N_TEXTURE_UPLOADS == uploads and map_textures.N_TEXTURE_BUILDS == builds + 2    # one per resident slice of the name
        assert_same_bits(old._grids[0, 0], host, what)
        assert_same_bits(both._grids[1, 0], host, what + ", mixed texture")
        assert_same_bits(both._grids[0, 0], conveyor, what + ": the other slice is untouched")
        assert np.array_equal(bits_of(E.sdf_grid_texture("Moving")), bits_of(host))             # the host texture follows

    def bits_of(a):
        return np.asarray(a).view(np.uint32)

    updated(occ_b, host_b, "after an update from a host array")
    E.register_occupancy_map("Fresh", occ_b)
    after, fresh = x.clone().cuda(), x.clone().cuda()
    old.guide_steps(after, hard, 0, 5)
    _gc().hip_guide("Fresh", [[]]).guide_steps(fresh, hard, 0, 5)
    assert torch.equal(after, fresh) and not torch.equal(after, before)       # a live guide's next call is a fresh guide's on the new map
    updated(torch.from_numpy(occ_c).cuda(), E.occupancy_sdf_texture(occ_c), "after an update from a device tensor")
    assert np.array_equal(E.map_occupancy("Moving"), occ_c)
    E.register_occupancy_map("Fresh2", occ_c)
    after, fresh = x.clone().cuda(), x.clone().cuda()
    old.guide_steps(after, hard, 0, 5)
    _gc().hip_guide("Fresh2", [[]]).guide_steps(fresh, hard, 0, 5)
    assert torch.equal(after, fresh)


def test_sampler_round_and_mpd_call_on_an_occupancy_map(registry, test_map):
    """One MultiRobotSampler round (4 robots, 4 samples, T = 25) and one MPD call (8 samples) on the test map: finite outputs, and the
    free mask is the host texture's decision on the returned trajectories."""
    from mmd_amd import postprocess as post
    from mmd_amd.multi_robot import MultiRobotSampler
    from mmd_amd.planners import MPD
    occ, tex = test_map
    E.register_occupancy_map("Floor", occ)
    starts, goals = synth.start_goal_circle(4, 0.45)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    s = MultiRobotSampler(_gc().hip_model(25), starts, goals, env_id="Floor", n_samples=4)
    s.set_other_paths(paths)
    trajs = s.sample(seed=5)
    best = s.best_paths(trajs, paths)
    assert trajs.shape == (16, H, D) and torch.isfinite(trajs).all() and best.shape == (4, H, 2) and torch.isfinite(best).all()
    t = s.unnormalize(trajs).contiguous()
    free = _host_free_mask(tex, t.cpu().numpy())[1]
    assert np.array_equal(post.postprocess_batch(s.guide, t, n_robots=4, smooth=False).free_mask.cpu().numpy().astype(bool), free)
    assert s.last_n_free.cpu().tolist() == free.reshape(4, 4).sum(1).tolist()
    p = MPD(model_id="EnvHighways2D-RobotPlanarDisk", env_id="Floor", planner_alg="mmd", start_state_pos=torch.from_numpy(starts[1]),
            goal_state_pos=torch.from_numpy(goals[1]), device="cuda", seed=23, n_samples=8,
            model_state_dict=synth.synth_unet_state_dict(0), model_args=dict(n_diffusion_steps=25), trained_models_dir="")
    assert p.env_id == "Floor"
    res = p(torch.from_numpy(starts[1]), torch.from_numpy(goals[1]))
    assert res.trajs_final.shape == (8, H, D) and torch.isfinite(res.trajs_final).all() and torch.isfinite(res.trajs_iters).all()
    free = _host_free_mask(tex, res.trajs_iters[-1].cpu().numpy())[1]      # the split is taken on the un-smoothed final samples
    assert res.trajs_iters[-1].shape == (8, H, D)
    assert sorted(res.trajs_final_free_idxs.view(-1).tolist()) == np.flatnonzero(free).tolist()
    assert sorted(res.trajs_final_coll_idxs.view(-1).tolist()) == np.flatnonzero(~free).tolist()
