"""-m gpu: the round's pick (mmd_amd/csrc/round_pick.hip) at its decision edges, against its definition on the CPU
(tests/round_pick_model.py) on the inputs of tests/round_pick_cases.py, whose reach tests/test_round_pick_cases_host.py asserts on the
model alone.  Through mmd_round_pick_paths by ctypes, with guard words around every output and the scratch: n_free, idx and the free flags
(the scratch's second block) equal the model's, the paths are bitwise the model's un-normalisation of the picked sample, a count key equals
the model's integer and a cost key lies within (H + 2) 2^-24 of the float64 key; where MultiRobotSampler._pick can express the settings the
call is bitwise that chain too; a second call into the same buffers gives the same words.  Then the calls the library refuses, and the pick
behind the sampler: shards of a larger instance, local rounds, the layer-by-layer and the f16 model."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_forms as F                   # noqa: E402
import post_edge_cases as E              # noqa: E402
import round_pick_cases as K             # noqa: E402
import round_pick_model as M             # noqa: E402
from mmd_amd import synth                # noqa: E402

H, D = 64, 4
GUARD, G = 0x5A5A5A5A, 64                # the guard word and how many of them lie either side of a buffer
KEY_BOUND = (H + 2) * E.U24              # a cost key against float64, relative (test_gpu_post_edges.py's sum bound, for the one key)
_GUIDES = {}


def _guide(case):
    """the guide whose map / boundary fields the call reads: R robots on the case's maps, with its extra objects"""
    key = (case.maps, case.extra is not None)
    if key not in _GUIDES:
        import gpu_common
        from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity
        ids = list(case.maps) if len(set(case.maps)) > 1 else None
        xo = None if case.extra is None else {k: np.asarray(v).tolist() for k, v in case.extra.items()}
        _GUIDES[key] = GuideManagerTrajectoriesWithVelocity(gpu_common.dataset(), env_id=case.maps[0], n_robots=case.R, robot_env_ids=ids,
                                                            extra_objects=xo, device="cuda")
    return _GUIDES[key]


class _Outputs:
    """paths_out, idx, n_free and the scratch of a call of R robots x B samples, each between G guard words, guard-filled"""

    def __init__(self, R, B):
        self.R, self.n = R, R * B
        self.sizes = dict(paths=R * H * 2, idx=R, n_free=R, scratch=2 * R * B)
        self.buf = {k: torch.full((2 * G + m,), GUARD, dtype=torch.int32, device="cuda") for k, m in self.sizes.items()}

    def ptr(self, name):
        return self.buf[name].data_ptr() + 4 * G

    def words(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.buf.items()}

    def read(self):
        """-> dict(paths float32 [R, H, 2], idx, n_free int32 [R], key float32 [n], free uint8 [n]) after the guard check"""
        w = self.words()
        for k, m in self.sizes.items():
            assert (w[k][:G] == GUARD).all() and (w[k][G + m:] == GUARD).all(), f"guard words of {k} overwritten"
        body = {k: w[k][G:G + m] for k, m in self.sizes.items()}
        n = self.n
        tail = body["scratch"][n:].view(np.uint8)
        assert (tail[n:] == 0x5A).all(), "scratch beyond its two blocks written"
        return dict(paths=body["paths"].view(np.float32).reshape(self.R, H, 2), idx=body["idx"], n_free=body["n_free"],
                    key=body["scratch"][:n].view(np.float32), free=tail[:n])

    def untouched(self):
        return all((w == GUARD).all() for w in self.words().values())


def _request(case, out):
    """the mmd_round_pick of the case with `out`'s buffers -> (struct, what it points at)"""
    from mmd_amd import _lib, postprocess as post
    s, keep = _lib.RoundPick(), []
    if case.paths_all is not None:
        p = torch.from_numpy(np.ascontiguousarray(case.paths_all, np.float32)).cuda()
        keep.append(p)
        s.paths_all_dev, s.n_all = p.data_ptr(), p.shape[0]
    s.robot0 = case.robot0
    s.norm_min, s.norm_max = (C.c_float * 4)(*[float(v) for v in case.norm_min]), (C.c_float * 4)(*[float(v) for v in case.norm_max])
    s.num_interpolation = case.ni
    if case.ni:
        alpha = post.interpolation_alphas(case.ni)
        keep.append(alpha)
        s.alpha = alpha.ctypes.data_as(C.POINTER(C.c_float))
    s.margin, s.rr_margin = case.margin, case.rr_margin
    s.q_min, s.q_max = (C.c_float * 2)(*case.q_min), (C.c_float * 2)(*case.q_max)
    s.paths_out_dev, s.idx_out_dev, s.n_free_out_dev, s.scratch_dev = out.ptr("paths"), out.ptr("idx"), out.ptr("n_free"), out.ptr("scratch")
    return s, keep


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _old_pick(case, x):
    """MultiRobotSampler._pick -- un-normalise -> mmd_postprocess_trajs -> mmd_count_collisions -> mmd_select_best -> gather -- of the case's
    robots on its guide: the method itself, on an object that holds only what it reads (the normaliser, the sample count, whether there
    are other robots); a sampler of its own would tie robot0 and the robot count to a shard"""
    import gpu_common
    from mmd_amd.multi_robot import MultiRobotSampler
    s = MultiRobotSampler.__new__(MultiRobotSampler)
    s.dataset, s.n_samples = gpu_common.dataset(), case.B
    s.n_robots = case.paths_all.shape[0] if case.paths_all is not None else 1
    paths_all = torch.from_numpy(case.paths_all).cuda() if case.paths_all is not None else None
    paths, idx, n_free = s._pick(x, _guide(case), case.robot0, case.R, paths_all, None)
    torch.cuda.synchronize()
    return paths.cpu().numpy(), idx.cpu().numpy(), n_free.cpu().numpy()


def _run_and_compare(case):
    """the case through mmd_round_pick_paths, held to the model (and to _pick where it can express the case) -> the kernels' outputs"""
    from mmd_amd import _lib
    assert case.x.dtype == np.float32 and case.x.shape == (case.R * case.B, H, D)
    x = torch.from_numpy(case.x).cuda().contiguous()
    out = _Outputs(case.R, case.B)
    s, keep = _request(case, out)
    desc = _guide(case).desc()
    _lib.launch("mmd_round_pick_paths", x, C.byref(desc), C.byref(s), C.c_void_p(x.data_ptr()), case.R, case.B)
    got = out.read()
    first = out.words()
    free, key, idx, n_free, paths = K.model(case)
    tag = case.name
    assert got["n_free"].tolist() == n_free.tolist(), (tag, got["n_free"].tolist(), n_free.tolist())
    bad = np.nonzero(got["free"] != free.reshape(-1))[0]
    assert bad.size == 0, f"{tag}: {bad.size} of {free.size} free flags differ, first at sample {bad[:4].tolist()}"
    assert got["idx"].tolist() == idx.tolist(), (tag, got["idx"].tolist(), idx.tolist())
    assert np.array_equal(_bits(got["paths"]), _bits(paths)), tag
    want = key.reshape(-1)
    assert np.array_equal(np.isnan(got["key"]), np.isnan(want)), tag
    ok = ~np.isnan(want)
    if case.paths_all is not None:
        assert np.array_equal(got["key"][ok].astype(np.int64), want[ok].astype(np.int64)) and np.array_equal(got["key"], np.rint(got["key"])), tag
    else:
        err = np.abs(got["key"][ok].astype(np.float64) - want[ok])
        got["key_ratio"] = float(np.max(err / np.maximum(KEY_BOUND * want[ok], 1e-300), initial=0.0))
        assert np.all(err <= KEY_BOUND * want[ok]), (tag, float(err.max()), got["key_ratio"])
    if case.default_settings:
        old = _old_pick(case, x)
        assert np.array_equal(_bits(got["paths"]), _bits(old[0])) and got["idx"].tolist() == old[1].tolist() and \
            got["n_free"].tolist() == old[2].tolist(), tag
    # a second call into the same buffers: the same words, the guards untouched
    _lib.launch("mmd_round_pick_paths", x, C.byref(desc), C.byref(s), C.c_void_p(x.data_ptr()), case.R, case.B)
    out.read()
    second = out.words()
    assert all(np.array_equal(first[k], second[k]) for k in first), tag
    return got


EDGE_CASES = {
    "map_edge_ni0": lambda: K.map_edge_case(0), "map_edge_ni1": lambda: K.map_edge_case(1), "map_edge_ni5": lambda: K.map_edge_case(5),
    "map_edge_ni16": lambda: K.map_edge_case(16), "wall_ni0": lambda: K.wall_case(0), "wall_ni5": lambda: K.wall_case(5),
    "limits": K.limit_case, "rr_margin": K.margin_case, "phantom_cost": K.phantom_cost_case, "phantom_map": K.phantom_map_case,
    "extra_objects": K.extra_object_case,
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_family_equals_the_model(name):
    """a - e and the extra objects: map cell edges with 0, 1, 5 and 16 (= MAX_INTERP) interpolants at segments 0, 31, 62 and at the last
    support point, the workspace walls, the joint limits (on, inside, outside), the robot-robot margin with robot0 = 2 of 7 (an exact
    pair, the own path, another robot's path), the phantom segment from the last support point to the origin, extra spheres and boxes"""
    case = EDGE_CASES[name]()
    assert case.name == name
    got = _run_and_compare(case)
    if name == "rr_margin":
        B = case.B
        assert all(got["key"][r * B] >= H > got["key"][r * B + 1] for r in range(3))       # another robot's path; its own
    if name.startswith("phantom"):
        assert got["idx"].tolist() == [0] and got["n_free"].tolist() == [2]


def test_two_maps_each_robot_on_its_own():
    """3 robots on [E.MAP, EnvConveyor2D, E.MAP] with the same samples: robots 0 and 2 get equal flags, robot 1 its own map's"""
    case = K.two_map_case()
    got = _run_and_compare(case)
    f = got["free"].reshape(3, case.B)
    assert np.array_equal(f[0], f[2]) and (f[0] != f[1]).sum() >= 8


@pytest.mark.parametrize("kind", K.PICK_KINDS)
def test_pick_sizes_equal_the_model(kind):
    """B in (1, 7, 64, 65, 129, 200) x R in (1, 3) x free shares (0, 0.1, 1): the scan's second and third trips, R B no multiple of the
    four samples of a workgroup; counts with the best count shared either side of index 64, cost, bit-for-bit ties, NaN keys"""
    worst = max(_run_and_compare(case).get("key_ratio", 0.0) for case in K.pick_size_cases(kind))
    print(f"pick sizes, {kind}: worst cost key error / bound = {worst:.3f}")


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------
def _small_case():
    x = K.normalised(np.random.default_rng(5).uniform(-0.5, 0.5, (2 * 4, H, D)))
    return K.Case("refusals", x, (K.EMPTY, K.EMPTY), paths_all=K.far_paths(3))


REFUSALS = {
    "num_interpolation_17": lambda s, a: setattr(s, "num_interpolation", 17),
    "null_alpha_table": lambda s, a: setattr(s, "alpha", None),
    "null_paths_out": lambda s, a: setattr(s, "paths_out_dev", None),
    "null_idx_out": lambda s, a: setattr(s, "idx_out_dev", None),
    "null_scratch": lambda s, a: setattr(s, "scratch_dev", None),
    "robots_beyond_n_all": lambda s, a: setattr(s, "robot0", 2),
    "robot0_negative": lambda s, a: setattr(s, "robot0", -1),
    "no_robots": lambda s, a: a.__setitem__("n_robots", 0),
    "no_samples": lambda s, a: a.__setitem__("samples_per_robot", 0),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refused_calls_name_their_function_and_write_nothing(what):
    """argument checks only: the call returns non-zero, mmd_last_error names mmd_round_pick_paths, the guard-filled outputs stay as they were"""
    from mmd_amd import _lib
    lib = _lib.load()
    case = _small_case()
    x = torch.from_numpy(case.x).cuda()
    out = _Outputs(case.R, case.B)
    s, keep = _request(case, out)
    args = dict(n_robots=case.R, samples_per_robot=case.B)
    REFUSALS[what](s, args)
    desc = _guide(case).desc()
    rc = lib.mmd_round_pick_paths(C.byref(desc), C.byref(s), C.c_void_p(x.data_ptr()), args["n_robots"], args["samples_per_robot"],
                                  _lib.current_stream_ptr())
    assert rc != 0 and b"mmd_round_pick_paths" in lib.mmd_last_error(), (what, rc, lib.mmd_last_error())
    assert out.untouched(), what


@pytest.mark.parametrize("what", ["null_pick", "null_guide"])
def test_sample_loop_pick_refuses_a_missing_pick_or_guide(what):
    from mmd_amd import _lib
    lib = _lib.load()
    case = _small_case()
    x = torch.from_numpy(case.x).cuda()
    out = _Outputs(case.R, case.B)
    s, keep = _request(case, out)
    desc = _guide(case).desc()
    rc = lib.mmd_p_sample_loop_pick(None, None, C.byref(desc) if what == "null_pick" else None, C.c_void_p(x.data_ptr()), None, case.R, case.B,
                                    1, 0, 1, None, C.c_uint64(0), None, None, 0, C.byref(s) if what == "null_guide" else None,
                                    _lib.current_stream_ptr())
    assert rc != 0 and b"mmd_p_sample_loop_pick" in lib.mmd_last_error(), (what, rc, lib.mmd_last_error())
    assert out.untouched() and np.array_equal(x.cpu().numpy(), case.x), what


# ---- through the sampler ---------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    """bitwise, NaNs included"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _model(T, **unet_options):
    """gpu_common.hip_model's network with creation-time options of the device model (layered, precision)"""
    import cases
    import gpu_common
    if not unet_options:
        return gpu_common.hip_model(T)
    from mmd_amd.diffusion_model import GaussianDiffusionModel
    from mmd_amd.temporal_unet import TemporalUnet
    unet = TemporalUnet(state_dim=4, n_support_points=64, unet_input_dim=32, dim_mults=(1, 2, 4), **unet_options)
    unet.load_state_dict(cases.named_state_dict(0))
    return GaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True)


def _sampler(N, B=8, T=25, model=None, **kw):
    from mmd_amd.multi_robot import MultiRobotSampler
    starts, goals = synth.start_goal_circle(N, 0.8)
    return MultiRobotSampler(model if model is not None else _model(T), starts, goals, n_samples=B, **kw)


_UNSHARDED = {}


def _unsharded(N, seed):
    """(paths_all, the unsharded sampler's paths, last_idx, last_n_free) of one round of N robots against their straight lines"""
    if (N, seed) not in _UNSHARDED:
        paths_all = torch.from_numpy(synth.straight_line_paths(*synth.start_goal_circle(N, 0.8), H)).cuda()
        s = _sampler(N, n_streams=1)
        s.set_other_paths(paths_all)
        _, paths = s._sample_and_pick(paths_all, None, seed)
        torch.cuda.synchronize()
        _UNSHARDED[(N, seed)] = (paths_all, paths.clone(), s.last_idx.clone(), s.last_n_free.clone())
    return _UNSHARDED[(N, seed)]


@pytest.mark.parametrize("n_streams", [1, 2])
@pytest.mark.parametrize("rank,world_size", [(1, 2), (2, 3)])
def test_shard_picks_with_its_robot0(rank, world_size, n_streams):
    """rank 1 of 2 (robots 3 .. 5) and rank 2 of 3 (robots 4, 5) of N = 6 robots (a shard count must divide N), B = 8, T = 25, in one and
    two stream chunks: the native pick behind the loop is bitwise _pick on the returned samples, equals the model's, and gives the rows
    the unsharded sampler gives these robots for the same seed.  Every robot's samples start on its own straight line's first point, so
    a self that is not skipped changes its counts."""
    N, B, seed = 6, 8, 17
    paths_all, full_paths, full_idx, full_n_free = _unsharded(N, seed)
    s = _sampler(N, rank=rank, world_size=world_size, n_streams=n_streams)
    assert s.robot0 == rank * (N // world_size) > 0
    s.set_other_paths(paths_all)
    assert s._takes_native_pick(None)
    trajs, paths = s._sample_and_pick(paths_all, None, seed)
    want = s._pick(trajs, s.guide, s.robot0, s.n_local, paths_all, None)
    torch.cuda.synchronize()
    assert torch.isfinite(trajs).all()
    assert _bits_equal(paths, want[0]) and torch.equal(s.last_idx, want[1]) and torch.equal(s.last_n_free, want[2])
    rows = slice(s.robot0, s.robot0 + s.n_local)
    assert _bits_equal(paths, full_paths[rows]) and torch.equal(s.last_idx, full_idx[rows]) and torch.equal(s.last_n_free, full_n_free[rows])
    # the definition, and what the wrong self would count
    import cases
    nz = s.dataset.normalizer
    lo, hi = nz.mins.float().cpu().numpy(), nz.maxs.float().cpu().numpy()
    x, pa = trajs.cpu().numpy(), paths_all.cpu().numpy()
    free, key, idx, n_free, mpaths = M.pick(x, lo, hi, [cases.guide_params(K.EMPTY)] * s.n_local, 5, 0.05, (-1.0, -1.0), (1.0, 1.0), pa, s.robot0)
    assert s.last_idx.cpu().tolist() == idx.tolist() and s.last_n_free.cpu().tolist() == n_free.tolist()
    assert np.array_equal(_bits(paths.cpu().numpy()), _bits(mpaths))
    u = M.unnormalise(x, lo, hi)
    wrong = np.stack([M.collision_counts(u[r * B:(r + 1) * B, :, :2], pa, r, F.MARGIN) for r in range(s.n_local)])
    assert (wrong != key).any()


def _ab(run):
    """run(sampler) with the native pick and without -> the two lists of tensors, compared bitwise"""
    out = []
    for native in (True, False):
        out.append(run(native))
    torch.cuda.synchronize()
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert _bits_equal(a, b) if isinstance(a, torch.Tensor) else a == b, (a, b)


def test_local_rounds_pick_natively_the_same():
    """plan_rounds(local_rounds=True, max_rounds=2) at N = 5, B = 8, T = 25: round 1 re-plans from round 0's samples (run_local_inference);
    with the native pick and without, the trajectories, paths, last_idx, last_n_free and the result's counts are the same bits"""
    def run(native):
        s = _sampler(5)
        s._native_pick = native
        assert s._takes_native_pick(None) == native
        res = s.plan_rounds(local_rounds=True, max_rounds=2, seed=40)
        assert res.n_rounds == 2 and torch.isfinite(res.trajs).all()
        return [res.trajs.clone(), res.paths_local.clone(), s.last_idx.clone(), s.last_n_free.clone(), res.robot_counts.clone(),
                list(res.conflict_counts)]
    _ab(run)


@pytest.mark.parametrize("options", [dict(layered=True), dict(precision="f16")], ids=["layered", "f16"])
def test_other_models_pick_natively_the_same(options):
    """one plan_round at N = 5, B = 8, T = 25 on the layer-by-layer model (its chunks are forced to 1, n_streams = 2 asked all the same) and
    on the f16 model: the native pick against sample + best_paths, bitwise"""
    N = 5
    p0 = torch.from_numpy(synth.straight_line_paths(*synth.start_goal_circle(N, 0.8), H)).cuda()

    def run(native):
        s = _sampler(N, model=_model(25, **options), n_streams=2)
        s._native_pick = native
        assert s._takes_native_pick(None) == native
        trajs, paths = s.plan_round(p0, seed=50)
        assert torch.isfinite(trajs).all()
        return [trajs.clone(), paths.clone(), s.last_idx.clone(), s.last_n_free.clone()]
    _ab(run)
