"""A numpy model of the selection of the robots a many-robot round re-plans (include/mmd_amd.h: mmd_round_select), shared by the CPU test
that checks its properties and the GPU tests that compare the kernels with it word for word; and the instances those tests run on.

It builds on round_model.report: a robot's count is the number of records that name it (every (t, pair) counts once for each of its two
robots: mmd_path_conflicts_binned's robot_counts), its neighbours are the robots it shares a record with.

"conflicted" selects every robot with a count above 0.  "independent" runs `iters` Jacobi iterations of priority propagation: r beats j
iff counts[r] > counts[j], or the counts are equal and r < j; a robot is OUT at the start if its count is 0, else UNDECIDED; one iteration
reads the old states only -- an UNDECIDED robot becomes OUT if a neighbour is IN, else IN if every neighbour that beats it is OUT, else it
stays; selected = IN after the last iteration."""
import numpy as np

import round_model as R

H = 64
CONFLICTED, INDEPENDENT = 0, 1                       # MMD_REPLAN_*
UNDECIDED, IN, OUT = 0, 1, 2


def counts_of(rep, n):
    """int32 [n]: the records of `rep` that name each robot"""
    _, a, b, _ = rep
    return (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int32)


def neighbours_of(rep, n):
    """[set]: the robots each robot shares a record with"""
    _, a, b, _ = rep
    nb = [set() for _ in range(n)]
    for x, y in zip(a.tolist(), b.tolist()):
        nb[x].add(y)
        nb[y].add(x)
    return nb


def beats(counts, r, j):
    return counts[r] > counts[j] or (counts[r] == counts[j] and r < j)


def iterate(counts, nb, iters):
    """the states after `iters` Jacobi iterations"""
    state = np.where(np.asarray(counts) == 0, OUT, UNDECIDED).astype(np.int32)
    for _ in range(iters):
        new = state.copy()
        for r in np.nonzero(state == UNDECIDED)[0].tolist():
            if any(state[j] == IN for j in nb[r]):
                new[r] = OUT
            elif all(state[j] == OUT for j in nb[r] if beats(counts, j, r)):
                new[r] = IN
        state = new
    return state


def partition(selected, robot0, n_local, undecided=0):
    """(perm int32 [n]: the stable partition, selected ids ascending then the others ascending; header int32 [4]: the number selected,
    of them below robot0, of them in [robot0, robot0 + n_local), the robots left UNDECIDED)"""
    selected = np.asarray(selected, np.int32)
    ids = np.arange(len(selected), dtype=np.int32)
    perm = np.concatenate([ids[selected == 1], ids[selected == 0]]).astype(np.int32)
    header = np.int32([selected.sum(), selected[:robot0].sum(), selected[robot0:robot0 + n_local].sum(), undecided])
    return perm, header


def select(paths, mode, iters=8, robot0=0, n_local=None, margin=R.F.MARGIN, rep=None):
    """-> (selected int32 [n], perm int32 [n], header int32 [4]) of the paths [n, H, 2]"""
    n = len(paths)
    n_local = n - robot0 if n_local is None else n_local
    rep = R.report(paths, margin) if rep is None else rep
    counts = counts_of(rep, n)
    if mode == CONFLICTED:
        selected, undecided = (counts > 0).astype(np.int32), 0
    else:
        state = iterate(counts, neighbours_of(rep, n), iters)
        selected, undecided = (state == IN).astype(np.int32), int((state == UNDECIDED).sum())
    return (selected,) + partition(selected, robot0, n_local, undecided)


def is_independent(selected, nb):
    return all(not (selected[r] and selected[j]) for r in range(len(nb)) for j in nb[r])


# ---- instances ----------------------------------------------------------------------------------------------------------------------
def parked(points):
    """paths [n, H, 2]: robot k parked at points[k]"""
    p = np.asarray(points, np.float32)
    return np.ascontiguousarray(np.broadcast_to(p[:, None, :], (len(p), H, 2))).copy()


def _apart(n):
    """n points 0.3 apart on a row: nobody meets"""
    return [(-0.9 + 0.3 * (k % 6), -0.6 + 0.3 * (k // 6)) for k in range(n)]


def hand_cases():
    """{name: paths} of the hand cases, N <= 8; two robots are neighbours where the text says so: 0.1 apart, the margin is 0.105"""
    out = {}
    p = parked(_apart(4))
    p[2] = p[1]                                                         # one pair, equal counts (64 each): the lower id
    out["pair"] = p
    p = parked(_apart(5))
    p[1:4] = parked([(0.0, 0.5), (0.1, 0.5), (0.2, 0.5)])               # a chain 1 - 2 - 3: 2 alone has two neighbours
    out["chain"] = p
    p = parked(_apart(6))
    p[[1, 3, 4]] = parked([(0.0, 0.5), (0.1, 0.5), (0.05, 0.58)])       # a triangle: one of three
    out["triangle"] = p
    p = parked(_apart(8))
    p[[5, 0, 2, 6, 7]] = parked([(0.0, 0.5), (0.1, 0.5), (-0.1, 0.5), (0.0, 0.6), (0.0, 0.4)])     # a star, centre 5
    out["star"] = p
    p = parked(_apart(6))
    p[4, 0] = p[0, 0]                                                   # the only conflict of 0 and 4 is at t = 0,
    p[5, H - 1] = p[3, H - 1]                                           # of 3 and 5 at t = 63
    out["first_and_last_step"] = p
    out["none"] = parked(_apart(8))
    out["two"] = parked([(0.5, 0.5), (0.5, 0.58)])                      # N = 2, the smallest table
    return out


LATTICE_SEED = 1


def lattice(seed=LATTICE_SEED, nx=18, ny=17, pitch=0.11, movers=40):
    """306 robots parked on an 18 x 17 lattice of pitch 0.11 (above the 0.105 margin: nobody meets), robot id = column-major position; a
    seeded few dozen step onto a neighbour's point for a few time steps.  The only instance past the partition kernel's 256-robot chunk."""
    rng = np.random.default_rng(900 + seed)
    ix, iy = np.divmod(np.arange(nx * ny), ny)
    pts = np.stack([(ix - (nx - 1) / 2) * pitch, (iy - (ny - 1) / 2) * pitch], 1)
    p = parked(pts)
    n = nx * ny
    for r in rng.choice(n, movers, replace=False).tolist():
        dx, dy = ((1, 0), (-1, 0), (0, 1), (0, -1))[int(rng.integers(0, 4))]
        jx, jy = ix[r] + dx, iy[r] + dy
        if not (0 <= jx < nx and 0 <= jy < ny):
            continue
        t0, length = int(rng.integers(0, H - 6)), int(rng.integers(2, 6))
        p[r, t0:t0 + length] = p[jx * ny + jy, 0]
    return p
