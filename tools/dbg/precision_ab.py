"""A/B of TemporalUnet's two precisions (mmd_unet_options.precision: f32 = the two-piece f16x2 arithmetic, f16 = one fp16 piece per
operand) on one GPU, in ONE process, the two alternating repeat by repeat, device events around every timed block:
  forward:  mmd_unet_forward at n = 64, 512, 2048 trajectories (unet_kernel<1> / <2> / <4>), blocks of LAUNCHES launches
  MPD:      one planner call, B = 64 samples, T = 25 (EnvHighways2D, no constraints)
  round:    one headline round through MultiRobotSampler.plan_round (32 robots x 64 samples on EnvEmpty2D, T = 100, inter-robot term)
Every shape is warmed up first.  On every run the outputs are compared: an arm's repeats with the same inputs are bitwise equal to its
first, and the f16 forward stays within 1e-2 rel-L2 of the f32 one without being equal to it.  Spread = (max - min) / mean over an arm's
repeats.  MMD_AMD_LIB selects the .so.  Usage: python tools/dbg/precision_ab.py [--out FILE] [--repeats R] [--only f32]
(--only f32: the f32 arm alone, for a library that predates the option -- the parent commit's, through MMD_AMD_LIB)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from mmd_amd import synth, _lib
if os.environ.get("MMD_AMD_LIB"):
    _lib.LIB_PATH = os.environ["MMD_AMD_LIB"]
from mmd_amd.diffusion_model import GaussianDiffusionModel
from mmd_amd.multi_robot import MultiRobotSampler
from mmd_amd.temporal_unet import TemporalUnet

H, LAUNCHES = 64, 50
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        k = args.index(name)
        v = args[k + 1]
        del args[k:k + 2]
        return v
    return default


out_path, repeats, only = opt("--out", None), int(opt("--repeats", "5")), opt("--only", None)
ARMS = (only,) if only else ("f32", "f16")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    """device time of fn() in ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    m = sum(v) / len(v)
    return m, (max(v) - min(v)) / m


def row(label, unit, t, scale=1.0, extra=""):
    cells = []
    for a in ARMS:
        m, s = stats(t[a])
        cells.append(f"{a} {m * scale:10.2f} {unit} (spread {100 * s:4.1f} %)")
    ratio = ""
    if len(ARMS) == 2:
        (m32, s32), (m16, s16) = stats(t["f32"]), stats(t["f16"])
        verdict = "f16 faster beyond the spread" if m16 * (1 + s16) < m32 * (1 - s32) else \
            "f16 slower beyond the spread" if m16 * (1 - s16) > m32 * (1 + s32) else "within the spread"
        ratio = f"   f16 / f32 {m16 / m32:5.3f}  ({verdict})"
    say(f"{label:<28} " + "   ".join(cells) + ratio + extra)


def unet_of(precision):
    kw = {} if only else {"precision": precision}           # (a library without the option: the four-field options struct's default)
    u = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=32, dim_mults=(1, 2, 4), **kw)
    u.load_state_dict(synth.synth_unet_state_dict(0))
    return u


unets = {a: unet_of(a) for a in ARMS}
say(f"{torch.cuda.get_device_name(0)}; library {os.environ.get('MMD_AMD_LIB', 'default')}; {repeats} repeats per arm, alternating; forward blocks of "
    f"{LAUNCHES} launches; device events")

# ---- the forward
for n in (64, 512, 2048):
    x = torch.from_numpy(synth.synth_noise(300, (n, H, 4))).cuda()
    first = {}
    for a in ARMS:
        for _ in range(5):
            first[a] = unets[a](x, 41)
    if len(ARMS) == 2:
        d = float((first["f16"].double() - first["f32"].double()).norm() / first["f32"].double().norm())
        assert 1e-5 < d < 1e-2, d
    t = {a: [] for a in ARMS}

    def block(u):
        for _ in range(LAUNCHES):
            y = u(x, 41)
        return y
    for _ in range(repeats):
        for a in ARMS:
            ms, y = timed(lambda: block(unets[a]))
            assert torch.equal(y, first[a]), (n, a)
            t[a].append(ms / LAUNCHES * 1e3)
    row(f"forward n = {n}", "us", t, extra=f"   f16 vs f32 rel-L2 {d:.2e}" if len(ARMS) == 2 else "")

# ---- one MPD call
from mmd_amd.planners import MPD   # noqa: E402
starts, goals = synth.start_goal_circle(10, 0.45)
planners = {a: MPD(model_id="EnvHighways2D-RobotPlanarDisk", planner_alg="mmd", start_state_pos=torch.as_tensor(starts[1]),
                   goal_state_pos=torch.as_tensor(goals[1]), device="cuda", seed=18, n_samples=64, model_state_dict=synth.synth_unet_state_dict(0),
                   model_args=dict(n_diffusion_steps=25), trained_models_dir="", **({} if only else {"unet_precision": a})) for a in ARMS}
call = lambda a, seed: planners[a](torch.from_numpy(starts[1]), torch.from_numpy(goals[1]), seed=seed)   # noqa: E731
first = {}
for a in ARMS:
    for _ in range(3):
        first[a] = call(a, 700).trajs_iters
    assert torch.isfinite(first[a]).all()
t = {a: [] for a in ARMS}
for _ in range(repeats):
    for a in ARMS:
        ms, o = timed(lambda: call(a, 700))
        assert torch.equal(o.trajs_iters, first[a]), a
        t[a].append(ms)
row("MPD call B = 64, T = 25", "ms", t)

# ---- one headline round
R, B, T = 32, 64, 100
starts, goals = synth.start_goal_circle(R, 0.8)
samplers = {a: MultiRobotSampler(GaussianDiffusionModel(model=unets[a], variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True),
                                 starts, goals, env_id="EnvEmpty2D", n_samples=B, rank=0, world_size=1, device="cuda", inter_robot=True)
            for a in ARMS}
paths0 = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
first = {}
for a in ARMS:
    for _ in range(2):
        first[a] = samplers[a].plan_round(paths0, seed=1000)
    assert torch.isfinite(first[a][0]).all()
t = {a: [] for a in ARMS}
for _ in range(repeats):
    for a in ARMS:
        ms, (tr, best) = timed(lambda: samplers[a].plan_round(paths0, seed=1000))
        assert torch.equal(tr, first[a][0]) and torch.equal(best, first[a][1]), a
        t[a].append(ms)
row(f"headline round {R} x {B}, T = {T}", "ms", t)
say(f"{'':<28} " + "   ".join(f"{a} {R * B / (stats(t[a])[0] * 1e-3):10.0f} trajectories/s" for a in ARMS))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
