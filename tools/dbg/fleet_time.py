"""What an epoch of a world fleet costs on the device, needs one GPU (run it under `timeout`; one process):

    python tools/dbg/fleet_time.py [--apart | --persistent | --aside] [OUT.txt]

The world is world_route_time.py's: 2048 x 2048 cells, 300 random boxes, clearance world.OBSTACLE_MARGIN.  With N = 64 and N = 256 robots,
starts and distinct goals drawn from the cells that one routable cell reaches, random-init weights, T = 25, B = 4 samples per robot,
reach 180 and max_steps 360 (WorldFleet's defaults), plan(max_rounds = 2):
  fields    the one-off build in WorldFleet's constructor: device_distance_field over the whole grid, one field per goal -- ONE pass, wall
            time with a device synchronisation at both ends (it allocates 4 * nx * ny bytes per goal; it is not repeated);
  sub-goals WorldFleet.epoch_targets: the upload of the robots' cells, one launch of mmd_grid_window_goals, one copy back, the offsets;
  sampler   WorldRobotSampler's construction on the epoch's windows, with the cut of its window slices (the map set is released after
            every pass, so every pass cuts);
  rounds    its plan(max_rounds = 2, seed).
Then the seeded epoch (WorldFleet(seed_epochs=True)) next to the unseeded one, on the same fleet, sampler and windows, the legs
alternating inside every pass (unseeded rounds, then the seeded leg's four parts, 1 warm-up pass and the median of 5 as above):
  targets+samples  epoch_targets with seeding on: one launch of mmd_grid_window_goal_samples in place of mmd_grid_window_goals, the same
                   one copy back (the row next to it is the unseeded epoch_targets, timed in the same passes);
  seeds            device_window_seeds: the upload of the start and goal points and one launch of mmd_window_seeds, 64 iterations;
  trajs            WorldRobotSampler.trajs_from_global: torch operations;
  seeded rounds    plan_rounds_seeded(init_trajs, paths_local = the seeds' positions, local_rounds=True, 3 + 3 steps, max_rounds = 2, seed).
Before these are timed, robot 0's samples and seed are compared with window_goal_samples and window_seed on the downloaded field and
texture, word for word and bit for bit.
Then the sub-goals kept apart (WorldFleet(separation=)) next to the plain ones, on the same fleet, alternating inside every pass in the same
protocol:
  targets apart    epoch_targets with separation = SUBGOAL_SEPARATION = 23: device_subgoals_apart's restart call of 4 sweeps and its one
                   copy back, and 4 more sweeps with another copy while robots still moved (the row says how many sweeps ran); the row
                   next to it is the plain epoch_targets, timed in the same passes.
The timing fleet's starts are random cells, drawn with no regard to one another, so the leg switches the separation on behind the
constructor's refusal; starts in conflict only give clear = 0.  Before the leg is timed: every robot that was not held back has the plain
targets' words, and every k lies in [0, walked].  --apart runs the field build, the plain sub-goals and this leg only.
--persistent times what an epoch pays before it plans, for the fleet's default and for WorldFleet(persistent=True), the two legs
alternating inside every pass on the same fleet and the same epoch's targets (1 warm-up pass, the median of 5):
  sampler + window cut   the default's: a WorldRobotSampler built on the epoch's named windows, the map set of the pass before released;
  persistent setup       one mmd_fleet_epoch_frames launch, one mmd_sdf_grid_windows_moved launch and the sampler's internal move, with
                         its slot bound (constraints.framed_slot_bound), on ONE sampler built with own_windows=True before the passes.
                         Before every timed call the sampler's windows are parked, untimed, one cell away from the epoch's origins, so
                         that the timed move cuts every slice; a third leg parks only the second half of the robots, as if the first half
                         had arrived and stood still: the timed move then cuts N / 2 slices.
Before these are timed: after a setup, every robot's slice, offsets and hard conditions are a fresh named sampler's, bit for bit.  It runs
the field build and these legs only, and leaves out the comparisons with the numpy definitions below (the other modes make them).
--aside times WorldFleet.epoch_targets with step_aside=True (aside_reach 48, aside_steps 96: device_subgoals_apart's loop, then
mmd_grid_window_goals_aside's restart call of 4 sweeps with its copy back, and 4 more while its state still moved) next to the same call
with the separation alone, which is the parent commit's path unchanged, the two legs alternating inside every pass on the same fleet:
  as drawn        the random starts at reach 180: the row says how many robots are held and yield (at this scale, few or none);
  pairs staged    8 pairs of robots put where the rule works: the goals of robots 2 i and 2 i + 1 are c + (23, 0) and c for a cell c with a
                  free row, robot 2 i + 1 stands on c and robot 2 i on c - (23, 0), and the reach is 40, so that robot 2 i's walk ends
                  17 cells beyond c and every cell of it conflicts with the standing robot; both legs run at that reach, with aside_reach 40.
Before a leg is timed: every robot that neither moved aside nor was released has the words of the separation alone.  It runs the field
build and these legs only.
Before anything is timed: the field of robot 0's goal is compared with the numpy definition, and the sub-goals of every 8th robot with
window_goals on the downloaded fields, integer for integer.  Per repeated figure: 1 warm-up pass, then the median of 5 passes.  'gpu ms'
= HIP events around the pass on the current stream, 'wall ms' = perf_counter around the pass with a device synchronisation at both ends.
The weights are random-init: the figures say what the loop costs, nothing about planning quality, and no threshold or default depends
on them.

Prints the table; with OUT.txt also writes it there."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mmd_amd import environments as E, map_textures, world_fleet as F, world_routes as R          # noqa: E402
from mmd_amd.world import WorldRobotSampler                                                        # noqa: E402
from world_route_time import LINES, random_world, say, timed                                      # noqa: E402

T, B, ROUNDS, SEED = 25, 4, 2, 7


def alternating(fns, passes=5, warmup=1, preps=None):
    """[(median gpu ms, median wall ms)] of every fn, the fns run one after the other inside every pass; preps[i], where given, runs
    before fn i, untimed"""
    import statistics
    gpu, wall = [[] for _ in fns], [[] for _ in fns]
    for k in range(warmup + passes):
        for i, fn in enumerate(fns):
            if preps is not None and preps[i] is not None:
                preps[i]()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                gpu[i].append(e0.elapsed_time(e1))
                wall[i].append(1e3 * (time.perf_counter() - t0))
    return [(statistics.median(g), statistics.median(w)) for g, w in zip(gpu, wall)]


def seeded_leg(fleet, sampler_of, wtex, lo, hi, pick, n):
    """the seeded epoch next to the unseeded one of the same fleet (the module's docstring)"""
    fleet.seed_epochs = True
    t = fleet.epoch_targets(fleet.positions)
    _, origins_dev, summary_dev = F._split_words(t.words)
    build = lambda: F.device_window_seeds(wtex, lo, hi, t.samples, origins_dev, summary_dev, fleet.window, fleet.positions, t.points,      # noqa: E731
                                          fleet.clearance, fleet.smooth_iters)
    seeds, clear_min = build()
    f = int(fleet.fields[0])
    want = F.window_goal_samples(fleet.dist[f].cpu().numpy(), pick[0], fleet.field_goals[f], fleet.reach, fleet.max_steps, fleet.window)
    assert want[4] == R.ROUTE_OK and np.array_equal(t.samples[0].cpu().numpy(), want[5]), "robot 0's samples are not the definition's"
    seed0, cmin0 = F.window_seed(wtex.cpu().numpy(), lo, hi, want[5], want[1], fleet.window, fleet.positions[0], t.points[0], fleet.clearance,
                                 fleet.smooth_iters)
    assert np.array_equal(seeds[0].cpu().numpy().view(np.int32), seed0.view(np.int32)), "robot 0's seed is not the definition's"
    assert clear_min[0].cpu().numpy().view(np.int32) == np.float32(cmin0).view(np.int32)
    sampler = sampler_of()
    init = sampler.trajs_from_global(seeds)
    paths0 = seeds[..., :2].contiguous()
    kw = dict(local_rounds=True, n_noising_steps=fleet.n_noising_steps, n_denoising_steps=fleet.n_denoising_steps, max_rounds=ROUNDS, seed=SEED)

    def targets(on):
        fleet.seed_epochs = on
        fleet.epoch_targets(fleet.positions)
    legs = alternating([lambda: sampler.plan(max_rounds=ROUNDS, seed=SEED), lambda: targets(False), lambda: targets(True), build,
                        lambda: sampler.trajs_from_global(seeds), lambda: sampler.plan_rounds_seeded(init, paths_local=paths0, **kw)])
    plain, seeded = sampler.plan(max_rounds=ROUNDS, seed=SEED), sampler.plan_rounds_seeded(init, paths_local=paths0, **kw)
    map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda")
    names = ("unseeded rounds", "unseeded targets", "targets+samples", "seeds", "trajs", "seeded rounds")
    say(f"N = {n:3d} | one session, legs alternating | " + " | ".join(f"{k}: gpu {g:7.3f} ms, wall {w:7.3f} ms" for k, (g, w) in zip(names, legs)))
    say(f"N = {n:3d} | unseeded rounds: {plain.n_rounds} run, conflicts {plain.conflict_counts}; seeded rounds ({fleet.n_noising_steps} + "
        f"{fleet.n_denoising_steps} steps, {fleet.smooth_iters} smoothing iterations): {seeded.n_rounds} run, conflicts "
        f"{seeded.conflict_counts}; least clear_min {float(clear_min.min()):.4f} at clearance {fleet.clearance}")
    fleet.seed_epochs = False


def apart_leg(fleet, n):
    """the sub-goals kept apart next to the plain ones of the same fleet (the module's docstring)"""
    def targets(separation):
        fleet.separation = separation
        return fleet.epoch_targets(fleet.positions)
    plain, apart = targets(None), targets(F.SUBGOAL_SEPARATION)
    k, walked, clear = apart.summary[:, 0], apart.extra[:, 0], apart.extra[:, 1]
    kept = walked == k
    assert ((0 <= k) & (k <= walked)).all() and np.array_equal(walked, plain.summary[:, 0]), "k outside [0, walked]"
    assert np.array_equal(apart.cells[kept], plain.cells[kept]) and np.array_equal(apart.summary[kept], plain.summary[kept])
    legs = alternating([lambda: targets(None), lambda: targets(F.SUBGOAL_SEPARATION)])
    fleet.separation = None
    say(f"N = {n:3d} | one session, legs alternating | " + " | ".join(f"{name}: gpu {g:7.3f} ms, wall {w:7.3f} ms" for name, (g, w) in
                                                                       zip(("plain targets", "targets apart"), legs)))
    say(f"N = {n:3d} | separation {F.SUBGOAL_SEPARATION} cells: {apart.sweeps} sweeps run, {int((~kept).sum())} robots held back (most "
        f"{int((walked - k).max())} cells, {int(((k == 0) & (walked > 0)).sum())} to k = 0), {int((clear == 0).sum())} with clear = 0 (starts in "
        f"conflict); longest walk {int(walked.max())} cells")


ASIDE_PAIRS = 8


def aside_pairs(cells, reached, rng, n_pairs=ASIDE_PAIRS, sep=F.SUBGOAL_SEPARATION):
    """[(c - (sep, 0), c, c + (sep, 0))] for n_pairs cells c whose row is connected ground from c - sep to c + sep, the triples 3 sep apart:
    a robot that stands on c holds one that walks the row from the first cell to the last with a reach below 2 sep"""
    found = []
    while len(found) < n_pairs:
        c = cells[rng.integers(0, len(cells))]
        if sep <= c[0] < reached.shape[0] - sep and reached[c[0] - sep:c[0] + sep + 1, c[1]].all() and \
                all(max(abs(int(c[0]) - int(o[1][0])), abs(int(c[1]) - int(o[1][1]))) >= 3 * sep for o in found):
            found.append((c - np.asarray([sep, 0]), c, c + np.asarray([sep, 0])))
    return found


def aside_leg(fleet, pairs, lo, hi, shape, n):
    """epoch_targets with step_aside next to the separation alone, on the same fleet (the module's docstring)"""
    def targets(step_aside, positions):
        fleet.step_aside = step_aside
        return fleet.epoch_targets(positions)
    fleet.separation, fleet.aside_reach, fleet.aside_steps = F.SUBGOAL_SEPARATION, 48, 96
    staged = fleet.positions.copy()                          # the pairs staged: the odd robot on its goal, the even one 23 cells before it
    for i, (before, c, _) in enumerate(pairs):
        staged[2 * i], staged[2 * i + 1] = R.cell_centres(before[None], lo, hi, shape)[0], R.cell_centres(c[None], lo, hi, shape)[0]
    for what, positions, reach in (("as drawn, reach 180", fleet.positions, 180), ("pairs staged, reach 40", staged, 40)):
        fleet.reach, fleet.aside_reach = reach, min(48, reach)
        apart, aside = targets(False, positions), targets(True, positions)
        bits = aside.aside[:, 0]
        kept = (bits & (F.ASIDE_MOVED | F.ASIDE_RELEASED)) == 0
        assert np.array_equal(aside.cells[kept], apart.cells[kept]) and np.array_equal(aside.summary[kept], apart.summary[kept])
        assert np.array_equal(aside.extra, apart.extra) and np.array_equal(aside.origins, apart.origins)
        legs = alternating([lambda: targets(False, positions), lambda: targets(True, positions)])
        say(f"N = {n:3d} | {what} | one session, legs alternating | " + " | ".join(f"{name}: gpu {g:7.3f} ms, wall {w:7.3f} ms" for name, (g, w) in
                                                                                  zip(("targets apart", "targets aside"), legs)))
        say(f"N = {n:3d} | {what} | {apart.sweeps} sweeps of phase 1; held {int((bits & F.ASIDE_HELD != 0).sum())}, yield "
            f"{int((bits & F.ASIDE_YIELDS != 0).sum())}, moved aside {int((bits & F.ASIDE_MOVED != 0).sum())} (longest side step "
            f"{int(aside.aside[:, 1].max())} cells), released {int((bits & F.ASIDE_RELEASED != 0).sum())}")
    fleet.separation, fleet.step_aside, fleet.reach = None, False, 180


def persistent_leg(fleet, model, targets, n):
    """the default's per-epoch set-up next to the persistent one of the same fleet and epoch (the module's docstring)"""
    words = targets.words
    _, origins_dev, _ = F._split_words(words)
    points_dev, goals_dev = torch.from_numpy(fleet.positions).cuda(), torch.from_numpy(fleet.goal_points).cuda()
    line_a = torch.from_numpy(np.linspace(0.0, 1.0, 64, dtype=np.float32)).cuda()
    ends = (fleet.positions, targets.points)
    origins = targets.origins.astype(np.int32)
    away = np.where(origins[:, :1] > 0, origins - np.int32([1, 0]), origins + np.int32([1, 0])).astype(np.int32)     # one cell off, in the world
    half = away.copy()
    half[:n // 2] = origins[:n // 2]
    sampler = WorldRobotSampler(model, fleet.positions, targets.points, targets.offsets, env_id="Timed", n_samples=B, own_windows=True)
    made = []

    def construct():
        for s in made:
            map_textures.release_sdf_textures(sorted(set(s._window_ids)), "cuda")
        made[:] = [WorldRobotSampler(model, fleet.positions, targets.points, targets.offsets, env_id="Timed", n_samples=B)]

    def setup():
        offsets_dev, _, hard_first, hard_last, _ = F.device_epoch_frames("Timed", words, points_dev, goals_dev, line_a=line_a)
        sampler._move_on_device(ends, targets.offsets, origins, offsets_dev, hard_first, hard_last, origins_dev)
    builds = []
    for parked in (away, half):
        sampler._move_windows(parked)
        before = map_textures.N_TEXTURE_BUILDS
        setup()
        builds.append(map_textures.N_TEXTURE_BUILDS - before)
    construct()
    fresh = made[0]
    same = lambda a, b: bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())        # noqa: E731
    assert same(sampler.guide._grids[:, 0], fresh.guide._grids[fresh.guide._robot_map.long(), 0]), "a moved slice is not the named one"
    assert same(sampler.offsets, fresh.offsets) and all(same(sampler.hard_conds[k], fresh.hard_conds[k]) for k in (0, 63))
    assert (sampler.neighbor_slots, sampler.world_limits, sampler.world_grid) == (fresh.neighbor_slots, fresh.world_limits, fresh.world_grid)
    legs = alternating([construct, setup, setup], preps=[None, lambda: sampler._move_windows(away), lambda: sampler._move_windows(half)])
    names = (f"sampler + window cut ({len(set(fresh._window_ids))} windows)", f"persistent setup ({builds[0]} slices cut)",
             f"persistent setup, half arrived ({builds[1]} slices cut)")
    say(f"N = {n:3d} | one session, legs alternating | " + " | ".join(f"{k}: gpu {g:7.3f} ms, wall {w:7.3f} ms" for k, (g, w) in zip(names, legs)))
    say(f"N = {n:3d} | neighbor_slots {sampler.neighbor_slots}; one texture set [{n}, 1, 400, 400, 4] = {sampler.guide._grids.numel() * 4 / 2 ** 20:.0f} MiB "
        f"for the run, against {len(set(fresh._window_ids))} named slices allocated and cut per epoch")
    map_textures.release_sdf_textures(sorted(set(fresh._window_ids)), "cuda")
    sampler.release_windows()


def main():
    import gpu_common
    apart_only, persistent_only, aside_only = "--apart" in sys.argv, "--persistent" in sys.argv, "--aside" in sys.argv
    out = [a for a in sys.argv[1:] if a not in ("--apart", "--persistent", "--aside")]
    say(f"# device: {torch.cuda.get_device_name(0)}; 1 warm-up pass, median of 5 (the field build: one pass)")
    occ = random_world(1)
    E.register_world_map("Timed", occ)
    wtex = map_textures.device_world_texture("Timed", "cuda")
    lo, hi = E.world_map_limits("Timed")
    rng = np.random.Generator(np.random.PCG64(3))
    rt = R.routable_cells(wtex.cpu().numpy(), R.OBSTACLE_MARGIN)
    seed_cell = np.argwhere(rt)[rng.integers(0, int(rt.sum()))]
    reached = (R.device_distance_field(wtex, seed_cell[None])[0][0] != R.UNREACHED).cpu().numpy()
    cells = np.argwhere(reached)
    say(f"world  {occ.shape[0]} x {occ.shape[1]} cells ({100 * occ.mean():.1f} % occupied), {int(rt.sum())} routable cells at clearance "
        f"{R.OBSTACLE_MARGIN}, {len(cells)} of them connected to cell {seed_cell.tolist()}; T = {T}, B = {B}, plan(max_rounds = {ROUNDS})")
    model = gpu_common.hip_model(T)
    for n in (64, 256):
        pick = cells[rng.choice(len(cells), 2 * n, replace=False)]
        pairs = aside_pairs(cells, reached, rng) if aside_only else []
        for i, (_, c, beyond) in enumerate(pairs):
            pick[n + 2 * i], pick[n + 2 * i + 1] = beyond, c
        starts, goals = R.cell_centres(pick[:n], lo, hi, occ.shape), R.cell_centres(pick[n:], lo, hi, occ.shape)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fleet = F.WorldFleet(model, "Timed", starts, goals, n_samples=B)
        torch.cuda.synchronize()
        t_fields = 1e3 * (time.perf_counter() - t0)
        assert fleet.dist.shape[0] == n
        if persistent_only:
            say(f"N = {n:3d} | fields ({n} goals, {4 * n * occ.size / 2 ** 20:.0f} MiB): wall {t_fields:9.1f} ms | longest way "
                f"{int(fleet.start_distances.max())} cells")
            persistent_leg(fleet, model, fleet.epoch_targets(fleet.positions), n)
            del fleet
            torch.cuda.empty_cache()
            continue
        ref = R.grid_distance_field(rt, fleet.field_goals[fleet.fields[0]][None])
        assert np.array_equal(fleet.dist[int(fleet.fields[0])].cpu().numpy(), ref[0]), "the device field is not the definition's"
        targets = fleet.epoch_targets(fleet.positions)
        for r in range(0, n, 8):
            f = int(fleet.fields[r])
            want = F.window_goals(fleet.dist[f:f + 1].cpu().numpy(), pick[r:r + 1], [0], fleet.field_goals[f:f + 1], fleet.reach, fleet.max_steps,
                                  fleet.window)
            assert (targets.cells[r].tolist(), targets.origins[r].tolist(), targets.summary[r].tolist()) == \
                (want[0][0].tolist(), want[1][0].tolist(), want[2][0].tolist()), f"robot {r}'s sub-goal is not the definition's"
        g_gpu, g_wall = timed(lambda: fleet.epoch_targets(fleet.positions))
        if aside_only:
            say(f"N = {n:3d} | fields ({n} goals, {4 * n * occ.size / 2 ** 20:.0f} MiB): wall {t_fields:9.1f} ms | longest way "
                f"{int(fleet.start_distances.max())} cells | sub-goals: gpu {g_gpu:7.3f} ms, wall {g_wall:7.3f} ms")
            aside_leg(fleet, pairs, lo, hi, occ.shape, n)
            del fleet
            torch.cuda.empty_cache()
            continue
        if apart_only:
            say(f"N = {n:3d} | fields ({n} goals, {4 * n * occ.size / 2 ** 20:.0f} MiB): wall {t_fields:9.1f} ms | longest way "
                f"{int(fleet.start_distances.max())} cells | sub-goals: gpu {g_gpu:7.3f} ms, wall {g_wall:7.3f} ms")
            apart_leg(fleet, n)
            del fleet
            torch.cuda.empty_cache()
            continue
        made = []

        def construct():
            for s in made:
                map_textures.release_sdf_textures(sorted(set(s._window_ids)), "cuda")
            made[:] = [WorldRobotSampler(model, fleet.positions, targets.points, targets.offsets, env_id="Timed", n_samples=B)]
        c_gpu, c_wall = timed(construct)
        sampler = made[0]
        p_gpu, p_wall = timed(lambda: sampler.plan(max_rounds=ROUNDS, seed=SEED))
        res = sampler.plan(max_rounds=ROUNDS, seed=SEED)
        map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda")
        say(f"N = {n:3d} | fields ({n} goals, {4 * n * occ.size / 2 ** 20:.0f} MiB): wall {t_fields:9.1f} ms | epochs needed at most "
            f"{fleet.epoch_bound()}, longest way {int(fleet.start_distances.max())} cells | sub-goals: gpu {g_gpu:7.3f} ms, wall {g_wall:7.3f} ms | "
            f"sampler + window cut ({len(set(sampler._window_ids))} windows): gpu {c_gpu:8.2f} ms, wall {c_wall:8.2f} ms | rounds "
            f"({res.n_rounds} run, conflicts {res.conflict_counts}): gpu {p_gpu:8.2f} ms, wall {p_wall:8.2f} ms")
        seeded_leg(fleet, sampler_of=lambda: WorldRobotSampler(model, fleet.positions, targets.points, targets.offsets, env_id="Timed", n_samples=B),
                   wtex=wtex, lo=lo, hi=hi, pick=pick, n=n)
        apart_leg(fleet, n)
        made.clear()
        del fleet, sampler
        torch.cuda.empty_cache()
    E.unregister_world_map("Timed")
    if out:
        with open(out[0], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
