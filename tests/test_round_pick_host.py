"""CPU: which full rounds of MultiRobotSampler sample and pick in one native call (mmd_p_sample_loop_pick) and which keep sample +
best_paths -- the Python wiring alone, with a stub in the model's place that records what a sampling call was asked for.  No GPU, no library."""
import torch

from mmd_amd import _lib, synth
from mmd_amd.multi_robot import MultiRobotSampler
from mmd_amd.normalization import TrajectoryDatasetFacade

H, D = 64, 4
N, B = 3, 4


class StubModel:
    """the library side of a sampling call: records the round_pick request (or None) of every call and returns zeros"""
    takes_round_pick = True

    def __init__(self):
        self.requests = []

    def run_inference(self, context, hard_conds, n_samples=1, n_robots=1, round_pick=None, **kw):
        self.requests.append(round_pick)
        return torch.zeros(n_samples * n_robots, H, D)

    def run_local_inference(self, prev, n_noising, n_denoising, context, hard_conds, n_samples=1, n_robots=1, round_pick=None, **kw):
        self.requests.append(round_pick)
        return prev.clone()


def _bare(cls=MultiRobotSampler, constraint_table="dense"):
    """a sampler without its guide (whose maps live on a GPU): the fields a full round's sampling and pick read"""
    s = object.__new__(cls)
    s.model = StubModel()
    s.constraint_table = constraint_table
    s.n_robots, s.robot0, s.n_local, s.n_samples = N, 0, N, B
    s.rank, s.world_size, s.group = 0, 1, None
    s.device = torch.device("cpu")
    s.dataset = TrajectoryDatasetFacade(synth.NORM_MINS, synth.NORM_MAXS)
    s.guide = None
    s.hard_conds = {}
    s.n_guide_steps, s.t_start_guide, s.n_extra, s.n_streams = 2, 3, 1, 0
    s.inter_robot = True
    s.last_idx = s.last_n_free = None
    s.picked = []                                           # best_paths calls (the fallback), recorded by the stand-in below
    return s


class Recording(MultiRobotSampler):
    """the chain of launches behind best_paths replaced by a record of the call: best_paths itself is the base class's"""
    def _pick(self, trajs_normalized, guide, robot0, n_robots, paths_all, collision_table):
        self.picked.append((paths_all, collision_table))
        return torch.zeros(n_robots, H, 2), torch.zeros(n_robots, dtype=torch.int32), torch.zeros(n_robots, dtype=torch.int32)

    def _collision_table(self, paths_all):
        return "cell table"


def _paths():
    return torch.zeros(N, H, 2)


def test_plain_round_sends_the_request():
    s = _bare()
    assert s._takes_native_pick(None)
    trajs, paths = s._sample_and_pick(_paths(), None, seed=1)
    (rp,) = s.model.requests
    assert rp is not None and isinstance(rp.struct, _lib.RoundPick)
    st = rp.struct
    assert paths is rp.paths and tuple(paths.shape) == (N, H, 2) and s.last_idx is rp.idx and s.last_n_free is rp.n_free
    assert st.paths_out_dev == rp.paths.data_ptr() and st.idx_out_dev == rp.idx.data_ptr() and st.n_free_out_dev == rp.n_free.data_ptr()
    assert st.paths_all_dev == rp.paths_all.data_ptr() and st.n_all == N and st.robot0 == 0
    assert rp.scratch.numel() * rp.scratch.element_size() >= N * B * 8
    assert list(st.norm_min) == list(synth.NORM_MINS) and list(st.norm_max) == list(synth.NORM_MAXS)
    assert st.num_interpolation == 5 and abs(st.alpha[0] - 1 / 6) < 1e-6
    # no gathered paths, or a local re-plan round: still the one call
    s._sample_and_pick(None, None, seed=2)
    assert s.model.requests[1].struct.paths_all_dev is None
    s._sample_and_pick(_paths(), None, 3, prev_trajs=torch.zeros(N * B, H, D))
    assert s.model.requests[2] is not None
    # the private switch
    s._native_pick = False
    assert not s._takes_native_pick(None)


def test_subclass_with_its_own_frame_falls_back():
    class Framed(Recording):
        def _in_shared_frame(self, t, robot0, n_robots):
            return t

    s = _bare(Framed)
    assert not s._takes_native_pick(None)
    p = _paths()
    s._sample_and_pick(p, None, seed=1)
    assert s.model.requests == [None] and len(s.picked) == 1 and s.picked[0][0] is p and s.picked[0][1] is None


def test_world_sampler_falls_back():
    from mmd_amd.world import WorldRobotSampler
    assert not _bare(WorldRobotSampler)._takes_native_pick(None)


def test_binned_table_falls_back():
    s = _bare(Recording, constraint_table="binned")
    assert not s._takes_native_pick(None)
    s._sample_and_pick(_paths(), None, seed=1)
    assert s.model.requests == [None] and s.picked[0][1] == "cell table"        # (best_paths counts on the cell table, as before)
    assert not _bare(constraint_table="binned")._takes_native_pick(None)


def test_collision_table_given_falls_back():
    s = _bare(Recording)
    table = object()
    assert not s._takes_native_pick(table)
    assert not _bare()._takes_native_pick(table)
    s._sample_and_pick(_paths(), table, seed=1)
    assert s.model.requests == [None] and s.picked[0][1] is table


def test_model_that_does_not_know_the_request_falls_back():
    s = _bare()
    s.model = type("Other", (), {})()
    assert not s._takes_native_pick(None)
