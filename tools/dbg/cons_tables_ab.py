"""A/B of the constraint-table builders (csrc/cons_tables.hip) against another build of the library, needs one GPU:

    python tools/dbg/cons_tables_ab.py OTHER.so COPY_OF_OTHER.so [--fine]

Three libraries in ONE process: OTHER.so ("parent"), a second copy of that file under another name (its own dlopen handle: the
parent/parent yardstick of the session's spread) and this tree's; _lib._lib is pointed at one of them between blocks of calls, the Python
wrappers are this tree's for all three.  Every stage's outputs are compared word for word across the libraries before it is timed.  HIP
events around every call, blocks of 20 calls, the sides alternating, three repetitions with the order rotated; 32 local robots of N = 32,
128, 512 on random straight lines.  The three libraries write the SAME buffers (one RoundConstraints, torch's cached blocks): a table per
library puts each side at other addresses, which moved a 10 us figure by several tenths of a us.  Gate per line: new mean - parent mean <= the
spread of the parent's six figures.  --fine: the all-pairs figures again with three decimals, six repetitions, 0.4 s a side, and the C
entry points 200 times back to back between two events (the kernel's own time where the GPU is the bound).  Prints the tables."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mmd_amd import _lib, synth                                           # noqa: E402
from mmd_amd import multi_agent as ma                                     # noqa: E402
from mmd_amd import constraints as K                                      # noqa: E402
from mmd_amd.environments import LIMITS                                   # noqa: E402

H = 64
ARGS = [v for v in sys.argv[1:] if not v.startswith("--")]
if len(ARGS) != 2:
    sys.exit(__doc__)


def say(s):
    print(s, flush=True)


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in list(_lib._SIGNATURES.items()) + list(_lib._DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.mmd_abi_version() == _lib.ABI_VERSION
    return lib


LIBS = {"parentA": load(os.path.abspath(ARGS[0])), "parentB": load(os.path.abspath(ARGS[1])), "new": load(_lib.LIB_PATH)}
NAMES = list(LIBS)


def use(name):
    _lib._lib = LIBS[name]


def words(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def stages(n_all, n_local=32):
    """{stage: (call() -> tuple of tensors, per-library state factory or None)}"""
    rng = np.random.default_rng(n_all)
    st, go = (rng.uniform(-0.9, 0.9, (n_all, 2)).astype(np.float32) for _ in range(2))
    local = synth.straight_line_paths(st, go, H)
    paths = torch.from_numpy(local).cuda()
    off_np = rng.uniform(0.0, 4.0, (n_all, 2)).astype(np.float32)
    offsets = torch.from_numpy(off_np).cuda()
    gpaths = torch.from_numpy((local + off_np[:, None, :]).astype(np.float32)).cuda()
    slots = K.framed_slot_bound(offsets, 0, n_local)
    grid = K.bin_grid(LIMITS, K.VERTEX_CONSTRAINT_RADIUS)
    batches = [torch.cat((paths[k:k + 1], torch.zeros((1, H, 2), device="cuda")), -1).contiguous() for k in range(n_all)]
    pc = ma.PathConstraints(batches, [0] * n_all, 0)
    pc_slots, pc_table = pc.extent()[1], pc.table()
    use("parentA")
    shared = (K.RoundConstraints(n_all, 0, n_local, 32), K.binned_collision_table(paths, 0, n_local))   # ONE table for every library

    def rc(name):
        return shared

    def append(name):
        r, tb = rc(name)
        r.append_conflicts(paths, tb)
        return r.ell, r.fill, r.dropped

    def set_soft(name):
        r, _ = rc(name)
        r.set_soft(paths)
        return (r.ell.view(n_local, r.slots_per_robot, H, 4)[:, r.hard_slots:],)

    return {
        "soft_constraints_from_paths": (lambda name: K.soft_constraints_from_paths(paths, 0, n_local)[:4], None),
        "RoundConstraints.set_soft": (set_soft, None),
        "append_conflicts": (append, lambda name: rc(name)[0].reset()),
        f"framed_constraints_from_paths slots={slots}": (lambda name: tuple(t for t in K.framed_constraints_from_paths(gpaths, offsets, 0, n_local, slots) if torch.is_tensor(t)), None),
        "cell table first_step=0": (lambda name: K.bin_constraints_table(paths, K.VERTEX_CONSTRAINT_RADIUS, LIMITS, grid, 0), None),
        "cell table first_step=1": (lambda name: K.bin_constraints_table(paths, K.VERTEX_CONSTRAINT_RADIUS, LIMITS, grid, 1), None),
        f"PathConstraints.build slots={pc_slots}": (lambda name: pc.build(2e-2, n_slots=pc_slots, table=pc_table), None),
    }


def measure(stage_map, reps=3, budget_s=0.12, max_calls=2000):
    rows = {}
    for stage, (call, prep) in stage_map.items():
        # word-for-word first
        ref = None
        for name in LIBS:
            use(name)
            if prep:
                prep(name)
            got = [words(t).cpu().clone() for t in call(name)]
            if ref is None:
                ref = got
            else:
                assert len(ref) == len(got) and all(torch.equal(a, b) for a, b in zip(ref, got)), f"{stage}: {name} differs from parentA"
        figs = {name: [] for name in LIBS}
        for rep in range(reps):
            tot = {name: 0.0 for name in LIBS}
            cnt = {name: 0 for name in LIBS}
            order = list(LIBS)
            order = order[rep % 3:] + order[:rep % 3]
            t_end = time.perf_counter() + budget_s * 3
            while time.perf_counter() < t_end and min(cnt.values()) < max_calls:
                for name in order:
                    use(name)
                    evs = []
                    for _ in range(20):
                        if prep:
                            prep(name)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call(name)
                        e1.record()
                        evs.append((e0, e1))
                    torch.cuda.synchronize()
                    tot[name] += sum(a.elapsed_time(b) for a, b in evs)
                    cnt[name] += 20
            for name in LIBS:
                figs[name].append(1e3 * tot[name] / cnt[name])
        rows[stage] = figs
    return rows


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}")
    say("# us per call (HIP events around every call, blocks of 20, sides alternating, 3 repetitions); spread = largest - smallest of the "
        "parent's six figures; gate: new mean - parent mean <= spread")
    say(f"{'figure':58s} {'parent A (3 reps)':>24s} {'parent B (3 reps)':>24s} {'new (3 reps)':>24s} | parent mean  spread  new mean  new - parent")
    outside = total = 0
    for n_all in (32, 128, 512):
        sm = stages(n_all)
        # warm-up: every stage once on every library
        for stage, (call, prep) in sm.items():
            for name in LIBS:
                use(name)
                if prep:
                    prep(name)
                call(name)
        torch.cuda.synchronize()
        for stage, figs in measure(sm).items():
            six = figs["parentA"] + figs["parentB"]
            pm, spread, nm = float(np.mean(six)), max(six) - min(six), float(np.mean(figs["new"]))
            ok = nm - pm <= spread
            total += 1
            outside += 0 if ok else 1
            f3 = lambda v: " ".join(f"{x:7.2f}" for x in v)
            say(f"{'N=%d %s' % (n_all, stage):58s} {f3(figs['parentA']):>24s} {f3(figs['parentB']):>24s} {f3(figs['new']):>24s} | {pm:11.2f} {spread:7.2f} {nm:9.2f} {nm - pm:+12.2f}  {'ok' if ok else 'OUTSIDE'}")
    say(f"# => figures outside the spread: {outside} of {total}; every library's outputs were equal word for word on every stage and size")


def run(label, calls, reps=6, budget_s=0.4, block=20, back_to_back=0):
    """calls: {lib name: zero-argument callable}; per-call events, or `back_to_back` calls between two events"""
    figs = {n: [] for n in NAMES}
    for rep in range(reps):
        order = NAMES[rep % 3:] + NAMES[:rep % 3]
        tot = {n: 0.0 for n in NAMES}
        cnt = {n: 0 for n in NAMES}
        t_end = time.perf_counter() + 3 * budget_s
        while time.perf_counter() < t_end:
            for n in order:
                f = calls[n]
                if back_to_back:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(back_to_back):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    tot[n] += e0.elapsed_time(e1)
                    cnt[n] += back_to_back
                else:
                    evs = []
                    for _ in range(block):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        evs.append((e0, e1))
                    torch.cuda.synchronize()
                    tot[n] += sum(a.elapsed_time(b) for a, b in evs)
                    cnt[n] += block
        for n in NAMES:
            figs[n].append(1e3 * tot[n] / cnt[n])
    six = figs["parentA"] + figs["parentB"]
    pm, spread, nm = float(np.mean(six)), max(six) - min(six), float(np.mean(figs["new"]))
    ab = max(abs(a - b) for a, b in zip(figs["parentA"], figs["parentB"]))
    say(f"{label:58s} | {pm:11.3f} {spread:7.3f} {ab:24.3f} {nm:9.3f} {nm - pm:+12.3f}  {'ok' if nm - pm <= spread else 'OUTSIDE'}")


def fine():
    say("# second pass over the all-pairs figures: six repetitions, 0.4 s a side; 'x 200 back to back': the C entry point 200 times between two events")
    say(f"{'figure (us per call)':58s} | parent mean  spread largest |A - B| in a rep  new mean  new - parent")
    stream = C.c_void_p(_lib.raw_stream())
    for n_all in (32, 128, 512):
        n_local = 32
        rng = np.random.default_rng(n_all)
        st, go = (rng.uniform(-0.9, 0.9, (n_all, 2)).astype(np.float32) for _ in range(2))
        paths = torch.from_numpy(synth.straight_line_paths(st, go, H)).cuda()
        rcs = {}
        _lib._lib = LIBS["parentA"]
        shared = K.RoundConstraints(n_all, 0, n_local, 32)        # ONE table for the three libraries: the same addresses for every side
        for n in NAMES:
            rcs[n] = shared

        def py_soft(n):
            def f():
                _lib._lib = LIBS[n]
                K.soft_constraints_from_paths(paths, 0, n_local)
            return f

        def py_set(n):
            def f():
                _lib._lib = LIBS[n]
                rcs[n].set_soft(paths)
            return f

        ell, gso, gw, rgo = K.group_tensors(n_local * (n_all - 1), n_local, n_local, paths.device)

        def c_soft(n):
            fn, a = LIBS[n].mmd_soft_constraints_from_paths, (paths.data_ptr(), n_all, 0, n_local, H, 0.12, 0.02, ell.data_ptr(), gso.data_ptr(),
                                                              gw.data_ptr(), rgo.data_ptr(), stream)
            return lambda: fn(*a)

        def c_set(n):
            fn, a = LIBS[n].mmd_round_soft_from_paths, (paths.data_ptr(), n_all, 0, n_local, H, 32, 0.12, rcs[n].ell.data_ptr(), stream)
            return lambda: fn(*a)

        for label, mk, b2b in (("soft_constraints_from_paths", py_soft, 0), ("RoundConstraints.set_soft", py_set, 0),
                               ("mmd_soft_constraints_from_paths x 200 back to back", c_soft, 200),
                               ("mmd_round_soft_from_paths x 200 back to back", c_set, 200)):
            calls = {n: mk(n) for n in NAMES}
            for n in NAMES:
                for _ in range(5):
                    calls[n]()
            torch.cuda.synchronize()
            run(f"N={n_all} {label}", calls, back_to_back=b2b)


if __name__ == "__main__":
    main()
    if "--fine" in sys.argv:
        fine()
