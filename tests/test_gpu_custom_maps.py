"""-m gpu: custom maps (environments.register_map).  The SDF grid mmd_sdf_grid_build builds on the device is the host texture (torch
autograd, the definition; tests/test_custom_maps_host.py holds it to the reference and to the numpy model) bit for bit, and everything
that reads the resident texture -- guide, samplers, planners, post-processing, per-robot maps -- runs on a registered map as on a
shipped one.  environments.update_map rebuilds the resident texture in place."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, map_textures, synth      # noqa: E402
from oracle import mmd_oracle as O                               # noqa: E402
import cases                                                     # noqa: E402
import sdf_grid_model as M                                       # noqa: E402
from cases import H, D                                           # noqa: E402


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


def _gc():
    import gpu_common
    return gpu_common


def assert_same_bits(dev, host, what):
    """torch.equal on all four channels, and the same bits wherever a word is not a zero: the sign of a zero is the one thing the device
    grid does not take from the host (it writes +0; autograd leaves -0 = 0 * -1 where a field has a single primitive)."""
    host = torch.as_tensor(host)
    dev = dev.cpu()
    assert dev.shape == host.shape, (what, dev.shape, host.shape)
    bad = (dev.view(torch.int32) != host.view(torch.int32)) & ~((dev == 0) & (host == 0))
    assert not bool((dev.view(torch.int32) == -2 ** 31).any()), f"{what}: the device grid holds a -0"
    assert torch.equal(dev, host) and not bool(bad.any()), \
        f"{what}: {int(bad.any(-1).sum())} of {bad[..., 0].numel()} nodes differ, first at {torch.argwhere(bad)[:4].tolist()}"


def raw_device_grid(boxes, spheres, xs, ys):
    """mmd_sdf_grid_build on any node rows; NaN-filled guard nodes behind the grid must stay untouched."""
    box, sph = E.primitive_tables(boxes, spheres)
    nx, ny = len(xs), len(ys)
    buf = torch.full((nx * ny + 64, 4), float("nan"), device="cuda")
    box_d, sph_d = torch.from_numpy(box).cuda(), torch.from_numpy(sph).cuda()
    xs_d, ys_d = torch.as_tensor(xs).cuda().contiguous(), torch.as_tensor(ys).cuda().contiguous()
    _lib.launch("mmd_sdf_grid_build", buf, sph_d.data_ptr() if len(sph) else None, len(sph), box_d.data_ptr() if len(box) else None,
                len(box), xs_d.data_ptr(), nx, ys_d.data_ptr(), ny, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[nx * ny:]).all()), "wrote behind the grid"
    return buf[:nx * ny].view(nx, ny, 4)


FULL_MAPS = ("EnvHighways2D", "EnvConveyor2D", "EnvDropRegion2D", "none", "tie_map", "tie_map_no_spheres")


@pytest.mark.parametrize("name", FULL_MAPS)
def test_device_grid_is_host_texture_full_size(registry, name):
    """The full 400 x 400 grid through environments.device_sdf_grid.  A shipped map's primitives against the shipped host texture (built
    with torch.minimum(1, .), which never acts there); the test map holds every tie kind."""
    if name.startswith("Env"):
        boxes, spheres = E.map_primitives(name)
        host = E.sdf_grid_texture(name)
    else:
        boxes, spheres = ((), ()) if name == "none" else M.tie_map(name == "tie_map")
        E.register_map("FullSize", boxes, spheres)
        host = E.sdf_grid_texture("FullSize")
    dev = E.device_sdf_grid(boxes, spheres, "cuda")
    assert tuple(dev.shape) == (400, 400, 4) and dev.dtype == torch.float32 and dev.is_cuda
    assert_same_bits(dev, host, name)
    again = E.device_sdf_grid(boxes, spheres, "cuda", out=dev)           # out=: in place
    assert again.data_ptr() == dev.data_ptr()
    assert_same_bits(again, host, name + ", out=")


def _random_primitives(n_spheres, n_boxes, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    spheres = np.concatenate([rng.uniform(-1, 1, (n_spheres, 2)), rng.uniform(0.01, 0.2, (n_spheres, 1))], 1)
    boxes = np.concatenate([rng.uniform(-1, 1, (n_boxes, 2)), rng.uniform(0.01, 0.4, (n_boxes, 2))], 1)
    return boxes.astype(np.float32).tolist(), spheres.astype(np.float32).tolist()


def _small_cases():
    tb, ts = M.tie_map()
    b300, s300 = _random_primitives(300, 300, 91)
    b5, s5 = _random_primitives(5, 4, 92)
    return {
        # nx != ny and 960 nodes = 3 full workgroups + one of 192 threads: a transposed or mis-strided index shows
        "24x40": (tb, ts, torch.linspace(-1, 1, 24), torch.linspace(-0.9, 0.7, 40)),
        "1x1": (tb, ts, torch.tensor([0.25]), torch.tensor([0.7])),          # the node is the centre of the two identical spheres
        "300+300 on 64x64": (b300, s300, torch.linspace(-1, 1, 64), torch.linspace(-1, 1, 64)),
        "spheres only": ((), s5, torch.linspace(-1, 1, 33), torch.linspace(-1, 1, 31)),
        "boxes only": (b5, (), torch.linspace(-2, 2, 31), torch.linspace(-2, 2, 33)),     # reaches nodes whose box distance is >= 1
        "nothing": ((), (), torch.linspace(-1, 1, 7), torch.linspace(-1, 1, 5)),
    }


@pytest.mark.parametrize("case", ["24x40", "1x1", "300+300 on 64x64", "spheres only", "boxes only", "nothing"])
def test_device_grid_is_host_texture_small_shapes(case):
    boxes, spheres, xs, ys = _small_cases()[case]
    host = E.primitives_sdf_texture(boxes, spheres, xs, ys)
    model = M.sdf_grid(boxes, spheres, xs.numpy(), ys.numpy())
    assert np.array_equal(model, host), case                                        # the numpy model agrees on these shapes too
    assert_same_bits(raw_device_grid(boxes, spheres, xs, ys), host, case)
    if case == "1x1":
        assert host[0, 0].tolist() == [pytest.approx(-0.1), 0.0, 0.0, 0.0]
    if case == "boxes only":
        assert (host[..., 0] == 1).any() and (host[..., 0] < 1).any()
    if case == "nothing":
        assert (host == np.array([1, 0, 0, 0], np.float32)).all()


def _grid_params(name, cutoff=0.05):
    """GuideParams whose one SDF grid is the HOST texture of a registered map."""
    tex = torch.from_numpy(E.sdf_grid_texture(name))
    return O.GuideParams(norm_mins=cases.MINS, norm_maxs=cases.MAXS, sdf_grids=[(tex[..., 0].contiguous(), tex[..., 1:3].contiguous())],
                         cutoff_margin=cutoff)


def test_guide_20_steps_on_a_registered_map_teacher_forced(registry):
    """20 chained guide iterations (mmd_guide_steps with its chain output) on the registered test map, with the inputs and constraints of
    test_guide_20_steps_vs_oracle (tests/test_gpu_parity.py:402-415), every iteration against the oracle on the host texture restarted
    from the kernel's state before it.  Bound per iteration: the single-evaluation bound of tests/test_gpu_parity.py:284-286, max abs < 2e-6.

    Teacher-forced, not free-running: 20 chained iterations of hinges and nearest-cell lookups amplify rounding, and by how much depends
    on the map and the inputs.  On this map the oracle's own free-running result moves by 5.0e-4 rel-L2 (2 of 12 draws) when x is scaled
    by 1 + 1.2e-7 u, u uniform in [-1, 1] per element, and by up to 1.8e-4 on EnvHighways2D, so no free-running bound near the shipped-map
    test's 2e-4 says anything about the kernel here (it ends 4.97e-4 from the oracle with every iteration within 3.0e-7 of it)."""
    E.register_map("TieMap", *M.tie_map())
    starts, goals, soft, hard = cases.highways_case()
    gp = _grid_params("TieMap")
    hc = cases.hard_conds_for(starts[3], goals[3])
    x = O.apply_hard_conditioning(torch.from_numpy(synth.synth_noise(50, (8, H, D))) * 0.5, hc)
    guide = _gc().hip_guide("TieMap", [[soft, hard]])
    assert guide.desc().n_grids == 1
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
    print(f"20 guide steps on the registered test map, teacher-forced: worst max abs {worst:.3e}")
    assert worst < 2e-6
    assert moved > 1e-3                                                      # the map's term acts on this batch


def test_guide_single_evaluation_on_a_registered_map_vs_oracle(registry):
    """One guide evaluation (mmd_guide_steps, one step, nothing pinned) on the registered test map against the oracle on the host texture:
    the inputs and the bound of the single-evaluation check of test_guide_and_postprocess_with_two_sdf_grids (tests/test_gpu_parity.py:279-286,
    max abs < 2e-6).  One evaluation has no chain of decisions behind it, so it shows the map term itself."""
    E.register_map("TieMap", *M.tie_map())
    x = torch.from_numpy(synth.synth_noise(60, (8, H, D))) * 0.6
    guide = _gc().hip_guide("TieMap", [[]])
    got = guide.forward(x.cuda()).cpu()
    ref = O.guide_grad(x, _grid_params("TieMap"), [], clip_mode="always")
    err = float((got - ref).abs().max())
    print(f"one guide evaluation on the registered test map: max abs {err:.3e}")
    assert err < 2e-6
    assert float((ref - O.guide_grad(x, cases.guide_params("EnvEmpty2D"), [], clip_mode="always")).abs().max()) > 1e-3      # the map acts


def test_registered_copy_of_highways_equals_the_shipped_map_end_to_end(registry):
    """EnvHighways2D's boxes under another name: the sampler's trajectories and picks, and one MPD call, are those of the shipped name."""
    from mmd_amd import diffusion_model as dm
    from mmd_amd.multi_robot import MultiRobotSampler
    from mmd_amd.planners import MPD
    E.register_map("HighwaysCopy", E.map_primitives("EnvHighways2D")[0])
    starts, goals = synth.start_goal_circle(4, 0.45)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    out = {}
    for env_id in ("EnvHighways2D", "HighwaysCopy"):
        s = MultiRobotSampler(_gc().hip_model(25), starts, goals, env_id=env_id, n_samples=4)
        s.set_other_paths(paths)
        trajs = s.sample(seed=5)
        best = s.best_paths(trajs, paths)
        out[env_id] = (trajs, best, s.last_idx, s.last_n_free)
    for a, b in zip(out["EnvHighways2D"], out["HighwaysCopy"]):
        assert torch.equal(a, b)
    assert torch.isfinite(out["HighwaysCopy"][0]).all() and out["HighwaysCopy"][0].shape == (16, H, D)
    res, draws = {}, dm._GLOBAL_DRAWS
    for env_id in ("EnvHighways2D", "HighwaysCopy"):
        dm._GLOBAL_DRAWS = draws                                  # the same point of the planners' global noise stream for both calls
        p = MPD(model_id="EnvHighways2D-RobotPlanarDisk", env_id=env_id, planner_alg="mmd", start_state_pos=torch.from_numpy(starts[1]),
                goal_state_pos=torch.from_numpy(goals[1]), device="cuda", seed=23, n_samples=8,
                model_state_dict=synth.synth_unet_state_dict(0), model_args=dict(n_diffusion_steps=25), trained_models_dir="")
        assert p.env_id == env_id
        res[env_id] = p(torch.from_numpy(starts[1]), torch.from_numpy(goals[1]))
    a, b = res["EnvHighways2D"], res["HighwaysCopy"]
    assert torch.equal(a.trajs_iters, b.trajs_iters) and torch.equal(a.trajs_final, b.trajs_final)
    assert torch.equal(a.trajs_final_free_idxs, b.trajs_final_free_idxs) and torch.equal(a.trajs_final_coll_idxs, b.trajs_final_coll_idxs)
    assert (a.idx_best_traj is None) == (b.idx_best_traj is None) and (a.idx_best_traj is None or int(a.idx_best_traj) == int(b.idx_best_traj))


def _nearest_cell_collides(tex, px, py, margin):
    """PlanningTask.compute_collision on the grid (grid_map_sdf.py:84-99, tasks.py:204-232) in numpy fp32: nearest cell of the host
    texture or a workspace boundary (1.08 x the limits, tasks.py:81-83) nearer than margin."""
    f = np.float32
    n = f(tex.shape[0])
    ix = np.clip(np.floor((px - f(-1)) / f(2) * n).astype(np.int64), 0, tex.shape[0] - 1)
    iy = np.clip(np.floor((py - f(-1)) / f(2) * n).astype(np.int64), 0, tex.shape[1] - 1)
    lo, hi = f(-1) * f(1.08), f(1) * f(1.08)
    return (tex[ix, iy, 0] < margin) | (px - lo < margin) | (py - lo < margin) | (hi - px < margin) | (hi - py < margin)


def test_postprocess_on_the_test_map_is_the_host_textures_nearest_cell(registry):
    from mmd_amd import postprocess as post
    E.register_map("TieMap", *M.tie_map())
    tex = E.sdf_grid_texture("TieMap")
    guide = _gc().hip_guide("TieMap", [[]])
    f = np.float32
    # straight lines through the big sphere and the thin box, beside them (surface + margin +- a little), and clear of everything
    ends = [((-0.9, 0.55), (0.9, 0.55)), ((-0.9, -0.4), (0.9, -0.42)), ((-0.313, -0.9), (-0.313, 0.9)), ((0.5, -0.9), (0.51, 0.9)),
            ((-0.9, 0.72), (-0.2, 0.722)), ((-0.9, 0.7195), (-0.2, 0.7195)), ((-0.9, 0.7205), (-0.2, 0.7205)), ((-0.8, -0.33), (0.1, -0.33)),
            ((-0.8, -0.3305), (0.1, -0.3295)), ((-0.9, 0.3), (0.9, 0.3)), ((-0.9, -0.9), (-0.2, -0.9)), ((0.9, 0.0), (0.6, 0.5)),
            ((-0.95, 0.2), (0.9, 0.25)), ((-0.7, 0.85), (-0.95, 0.6)), ((0.0, -0.2), (0.0, -0.6)), ((0.3, -0.1), (0.9, -0.2))]
    w = np.linspace(0, 1, H, dtype=np.float32)[:, None]
    trajs = np.zeros((len(ends), H, 4), np.float32)
    for k, (a, b) in enumerate(ends):
        trajs[k, :, :2] = np.asarray(a, f) * (f(1) - w) + np.asarray(b, f) * w
    alpha = post.interpolation_alphas(5)
    px = trajs[:, :-1, None, 0] * alpha + trajs[:, 1:, None, 0] * (f(1) - alpha)
    py = trajs[:, :-1, None, 1] * alpha + trajs[:, 1:, None, 1] * (f(1) - alpha)
    want = _nearest_cell_collides(tex, px, py, f(post.ROBOT_RADIUS)).reshape(len(ends), -1)
    free = ~want.any(1)
    assert free.any() and not free.all() and want[0].any() and want[1].any()
    r = post.postprocess_batch(guide, torch.from_numpy(trajs).cuda(), num_interpolation=5, smooth=False, want_waypoints=True)
    assert np.array_equal(r.waypoint_collisions.cpu().numpy().astype(bool), want)
    assert np.array_equal(r.free_mask.cpu().numpy().astype(bool), free)
    pts = np.random.Generator(np.random.PCG64(93)).uniform(-1, 1, (4096, 2)).astype(np.float32)
    occ = post.compute_collision(torch.from_numpy(pts).cuda(), guide, margin=0.05).cpu().numpy()
    assert np.array_equal(occ, _nearest_cell_collides(tex, pts[:, 0], pts[:, 1], f(0.05))) and occ.any() and not occ.all()


def test_per_robot_maps_mix_shipped_and_registered(registry):
    """robot_env_ids = a shipped and a registered name in one guide: each robot's rows are the single-map guide's."""
    E.register_map("TieMap", *M.tie_map())
    B = 4
    x = torch.from_numpy(synth.synth_noise(94, (3 * B, H, D))) * 0.6
    hard = torch.zeros(3, 2, D, device="cuda")
    env_ids = ["EnvHighways2D", "TieMap", "EnvHighways2D"]
    mixed = _gc().hip_guide("EnvEmpty2D", [[], [], []], n_robots=3, robot_env_ids=env_ids)
    assert mixed._grids.shape[0] == 2 and mixed.desc().n_grids == 1
    y = x.clone().cuda()
    mixed.guide_steps(y, hard, 0, 5)
    singles = {}
    for r, env_id in enumerate(env_ids):
        z = x[r * B:(r + 1) * B].clone().cuda()
        _gc().hip_guide(env_id, [[]]).guide_steps(z, hard[:1].contiguous(), 0, 5)
        assert torch.equal(y[r * B:(r + 1) * B], z), (r, env_id)
        singles[r] = z
    x1 = x[:B].clone().cuda()
    _gc().hip_guide("TieMap", [[]]).guide_steps(x1, hard[:1].contiguous(), 0, 5)
    assert not torch.equal(x1, singles[0])                                   # the two maps act differently on the same rows


def test_update_map_rebuilds_the_resident_texture_in_place(registry):
    boxes_a, spheres_a = [(0.0, 0.0, 0.6, 0.3)], [(-0.5, 0.5, 0.2)]
    boxes_b, spheres_b = M.tie_map()
    E.register_map("Moving", boxes_a, spheres_a)
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
    uploads, builds = map_textures.N_TEXTURE_UPLOADS, map_textures.N_TEXTURE_BUILDS
    E.update_map("Moving", boxes_b, spheres_b)
    assert (old._grids.data_ptr(), both._grids.data_ptr()) == ptrs
    assert map_textures.N_TEXTURE_UPLOADS == uploads and map_textures.N_TEXTURE_BUILDS == builds + 2        # one per resident slice of the name
    host_b = E.sdf_grid_texture("Moving")
    assert_same_bits(old._grids[0, 0], host_b, "after the update")
    assert_same_bits(both._grids[1, 0], host_b, "after the update, mixed texture")
    assert_same_bits(both._grids[0, 0], E.sdf_grid_texture("EnvConveyor2D"), "the other slice is untouched")
    E.register_map("Fresh", boxes_b, spheres_b)
    after, fresh = x.clone().cuda(), x.clone().cuda()
    old.guide_steps(after, hard, 0, 5)
    _gc().hip_guide("Fresh", [[]]).guide_steps(fresh, hard, 0, 5)
    assert torch.equal(after, fresh) and not torch.equal(after, before)
