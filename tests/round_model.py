"""A numpy model of the round table's hard block (include/mmd_amd.h: mmd_conflict_constraints_append), shared by the CPU test that pins it
to mmd_pack_constraints and the GPU tests that compare the kernels with it; and the instances those tests run on.

The slot rule: a robot's points arrive in report order, point (tc, mid) has range (tc - t_pad, tc + t_pad), i.e. it is active at the
integer t with tc - t_pad <= t < tc + t_pad inside [0, H); its slot at t is the number of earlier points active at t (mmd_pack_constraints'
rule).  A point whose slot would reach the cap is not written at that t and counts as dropped there."""
import numpy as np

import fp32_forms as F

H = 64
RADIUS = np.float32(0.05 * 2.4)                      # constraints.VERTEX_CONSTRAINT_RADIUS as the fp32 the kernels are passed
INACTIVE = np.array([0.0, 0.0, -1.0, -1.0], np.float32)


class HardBlock:
    """One robot's hard block: ell [cap, H, 4] float32, fill [H], dropped; append() keeps the state, as the device arrays do."""

    def __init__(self, cap, radius=RADIUS):
        self.cap, self.radius = int(cap), np.float32(radius)
        self.ell = np.tile(INACTIVE, (self.cap, H, 1))
        self.fill = np.zeros(H, np.int32)
        self.count = np.zeros(H, np.int64)           # the points active at t, kept or not
        self.dropped = 0

    def append(self, tc, mid, t_pad=2):
        word = np.float32(self.radius) * np.abs(np.float32(self.radius))
        for c, q in zip(np.asarray(tc, np.int64), np.asarray(mid, np.float32).reshape(-1, 2)):
            for t in range(max(int(c) - t_pad, 0), min(int(c) + t_pad, H)):
                if self.count[t] < self.cap:
                    self.ell[self.count[t], t] = (q[0], q[1], self.radius, word)
                    self.fill[t] += 1
                else:
                    self.dropped += 1
                self.count[t] += 1
        return self


def report(paths, margin=F.MARGIN):
    """The conflict report of paths [N, H, 2] float32 in numpy: (t, a, b, mid [m, 2]) of every a < b with ||p_a(t) - p_b(t)|| < margin in
    the pinned fp32 form, row-major in (t, a, b); mid = (p_a + p_b) / 2 in fp32 (mmd_path_conflicts_binned's records)."""
    p = np.ascontiguousarray(np.transpose(np.asarray(paths, np.float32), (1, 0, 2)))     # [T, N, 2]
    hit = F.pos_norm(p[:, :, None, :], p[:, None, :, :]) < np.float32(margin)
    t, a, b = np.nonzero(np.triu(hit, 1))
    mid = (p[t, a] + p[t, b]) / np.float32(2)
    return t, a, b, mid.astype(np.float32)


def robot_points(rep, robot):
    """(tc, mid) of the records of `rep` that name `robot`, in report order"""
    t, a, b, mid = rep
    m = (a == robot) | (b == robot)
    return t[m], mid[m]


def blocks(reports, robot0, n_local, cap, t_pad=2, radius=RADIUS):
    """[HardBlock] of the local robots after the reports of successive rounds"""
    out = []
    for r in range(n_local):
        blk = HardBlock(cap, radius)
        for rep in reports:
            blk.append(*robot_points(rep, robot0 + r), t_pad=t_pad)
        out.append(blk)
    return out


def max_fill(reports, n_all, t_pad=2):
    """the largest number of points any robot has active at one time step (an uncapped block's largest fill)"""
    return max(int(b.count.max()) for b in blocks(reports, 0, n_all, 1, t_pad))


# ---- instances ----------------------------------------------------------------------------------------------------------------------
def instance_a():
    """A: 6 robots on the r = 0.8 circle with antipodal goals, straight lines -- everyone meets at the centre"""
    from mmd_amd import synth
    starts, goals = synth.start_goal_circle(6, 0.8)
    return starts, goals, synth.straight_line_paths(starts, goals, H)


def instance_b(seed=0, n=48, meet_outside=False):
    """B: 48 robots on seeded random walks in [-1, 1]^2, with coincident robots, robots a few ulps either side of the margin from
    another (at every time step), and a robot parked outside the limits; each kind also inside the shard [16, 32).  meet_outside: a
    second robot joins the parked one, so that there are conflicts outside the limits too (table tests only: a normalised sample cannot
    lie out there, so no constraint at that place acts on one)"""
    rng = np.random.default_rng(600 + seed)
    p = np.empty((n, H, 2), np.float64)
    p[:, 0] = rng.uniform(-0.9, 0.9, (n, 2))
    for t in range(1, H):
        p[:, t] = np.clip(p[:, t - 1] + rng.normal(0.0, 0.03, (n, 2)), -1.0, 1.0)
    p = p.astype(np.float32)
    p[8] = p[7]                                                      # coincident
    p[25] = p[24]
    for k, anchor in ((3, 2), (18, 17), (30, 5), (40, 29)):          # at the margin, both sides
        p[k] = F.near_points(rng, p[anchor], float(F.MARGIN))
    p[20] = (1.3, -1.2)                                              # parked outside the limits
    if meet_outside:
        p[21, 40:] = (1.3, -1.2)
    return p


def instance_b_next():
    """another round's paths for the same 48 robots (the append tests)"""
    return instance_b(seed=1, meet_outside=True)
