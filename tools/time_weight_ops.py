"""dev aid (GPU box): what class weights and balanced epochs cost (csrc/kernels_weights.h, the _cw criteria, device_data.py:
BalancedEpochSampler) at cfg4's shapes: B = 256, T = 60, C = 4, the distance graph, the whole step captured with include_update.
    (a) default_step     the step WITHOUT weights of this tree against another build of the library (--lib PARENT.so, the parent
                         commit's): the same kernels, so any difference beyond the spread of parent-against-parent -- two captures
                         under the parent's library, measured in the same call -- wants an explanation.  The first loss of every
                         capture is bit-compared.
    (b) weighted_step    the same step with TrainStep(class_weights=...): one more launch (clip_weights) and the _cw head.  And per
                         launch: `clip_weights` (batch form and sampler form), the fused head plain / _w / _cw, `ce_logits` plain /
                         _w / _cw.
    (c) begin_epoch      `BalancedEpochSampler.begin_epoch` against `EpochSampler.begin_epoch` at a pool of 100 000 clips with 5 %
                         positives (host clock around --epochs calls, ending in a synchronise).
Every step runs in a process of its own under its own time limit (--limit seconds); the first step that fails or runs out of time
ends the run.  Inside a step every candidate is warmed, then --rounds rounds alternate between the candidates; median and spread
(min..max) over the rounds.
usage: python tools/time_weight_ops.py --lib PARENT.so [--rounds 7] [--out profiles/class_weights.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so (the parent commit's) whose default step is timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20, help="step replays per timed sample")
ap.add_argument("--launches", type=int, default=200, help="launches per timed sample of a kernel")
ap.add_argument("--epochs", type=int, default=20, help="begin_epoch calls per timed sample")
ap.add_argument("--pool", type=int, default=100000)
ap.add_argument("--limit", type=int, default=300, help="time limit of one step, seconds")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["steps", "ops"], help="(internal) run this one step and print its JSON line")
opt = ap.parse_args()
if opt.rounds < 7:
    sys.exit("time_weight_ops: at least 7 rounds")

STEPS = ("steps", "ops")
CLASS_W = [0.5, 1.0, 2.0, 4.0]


def driver():
    """every step in a fresh process under its own time limit; stop at the first failure"""
    results = {}
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [a for a in sys.argv[1:] if a != "--step"]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"time_weight_ops: step {step!r} ran past its limit of {opt.limit} s; nothing further is started")
        if done.returncode != 0:
            sys.exit(f"time_weight_ops: step {step!r} ended with status {done.returncode}; nothing further is started")
        results[step] = json.loads(done.stdout.strip().splitlines()[-1])
    text = "\n".join(report(results))
    print(text)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(text + "\n")


def report(res):
    st, op = res["steps"], res["ops"]
    fmt = lambda v: f"{v[0]:10.3f} ({v[1]:10.3f} .. {v[2]:10.3f})"     # noqa: E731
    lines = [f"device: {st['device']}; cfg4 shapes: B = 256, T = 60, C = 4, distance graph, the whole step captured (include_update); rounds = "
             f"{opt.rounds}, {opt.reps} replays per sample",
             "(a) + (b) ms per step (device events around the replays): median (min .. max), ratio to this tree's default step"]
    base = st["ms"]["default, this tree"][0]
    for name, v in st["ms"].items():
        lines.append(f"  {name:<34s} {fmt(v)}  {v[0] / base:6.4f}")
    if "default, other lib" in st["ms"]:
        a, b = st["ms"]["default, other lib"][0], st["ms"]["default, other lib (again)"][0]
        lines += [f"  this tree against the other library: {(base - a) / a * 100:+.3f} % of its median; the other library against itself (two "
                  f"captures): {(b - a) / a * 100:+.3f} %",
                  f"  first loss of every default capture, bit-compared with this tree's: {st['same_loss']}"]
    lines.append(f"  weighted step against this tree's default step: {(st['ms']['class weights, this tree'][0] - base) * 1e3:+.2f} us per step")
    lines.append(f"(b) us per launch (device events around {opt.launches} back-to-back launches; an eager launch includes its host side): median (min .. max)")
    for name, v in op["us"].items():
        lines.append(f"  {name:<34s} {fmt(v)}")
    lines.append(f"(c) ms per begin_epoch at a pool of {opt.pool} clips, 5 % positives (host clock around {opt.epochs} calls and a synchronise): "
                 f"median (min .. max); balanced epoch_len = {op['epoch_len']}")
    for name, v in op["epoch_ms"].items():
        lines.append(f"  {name:<34s} {fmt(v)}")
    return lines


def spread(v):
    return (statistics.median(v), min(v), max(v))


def events(torch, fn, n):
    """ms per call over n calls in a row"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def step_steps():
    import torch
    import bench
    from eeg_gnn_ssl_amd import DCRNNModel_classification, _lib
    from eeg_gnn_ssl_amd.train_step import TrainStep
    assert torch.cuda.is_available(), "time_weight_ops.py measures on an MI355X; there is no other path"
    dev = torch.device("cuda", 0)
    task, filt, t_len, batch, classes = bench.WORKLOADS["cfg4"]
    x, y, lengths, sup = bench.synthetic_batch(task, filt, t_len, batch, classes, seed=123)
    x, y, lengths, sup = x.to(dev), y.to(dev), lengths.to(dev), [s.to(dev) for s in sup]
    this = _lib.get_lib()
    other = _lib.EegDcrnnLib(os.path.abspath(opt.lib), strict=False) if opt.lib else None

    def captured(lib, **kw):
        """a step captured under `lib` -> (replay(), first loss): the graph keeps that library's kernels"""
        _lib._LIB = lib
        try:
            torch.manual_seed(123)
            model = DCRNNModel_classification(bench.make_args(filt), classes, device=dev).to(dev)
            model.train()
            st = TrainStep(model, task=task, lr=3e-4, weight_decay=5e-4, max_grad_norm=5.0, **kw)
            keep = st.snapshot()
            st.capture(x, y, lengths, sup, include_update=True)
            st.restore(keep)
            first = st.replay_step().clone()
        finally:
            _lib._LIB = this
        return st.replay_step, first

    cands = {"default, this tree": captured(this)}
    if other is not None:
        cands["default, other lib"] = captured(other)
        cands["default, other lib (again)"] = captured(other)
    cands["class weights, this tree"] = captured(this, class_weights=CLASS_W)
    same = all(bool(torch.equal(v[1], cands["default, this tree"][1])) for k, v in cands.items() if k.startswith("default"))
    for fn, _ in cands.values():
        events(torch, fn, 5)
    got = {name: [] for name in cands}
    for _ in range(opt.rounds):
        for name, (fn, _) in cands.items():
            got[name].append(events(torch, fn, opt.reps))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "same_loss": same, "ms": {k: spread(v) for k, v in got.items()}}))


def step_ops():
    import torch
    from eeg_gnn_ssl_amd import BalancedEpochSampler, EpochSampler, ops
    assert torch.cuda.is_available(), "time_weight_ops.py measures on an MI355X; there is no other path"
    dev = torch.device("cuda", 0)
    E = torch.ops.eeg_dcrnn
    g = torch.Generator(device=dev).manual_seed(7)
    b, n, h, c, pool = 256, 19, 64, 4, opt.pool
    z = torch.randn(b, n, h, generator=g, device=dev)
    w, bias = 0.3 * torch.randn(c, h, generator=g, device=dev), torch.zeros(c, device=dev)
    y = torch.randint(0, c, (b,), generator=g, device=dev)
    lg = torch.randn(b, c, generator=g, device=dev)
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    class_w = torch.tensor(CLASS_W, device=dev)
    clip_u, denom = torch.empty(b, device=dev), torch.empty(1, device=dev)
    ops.clip_weights(y, clip_u, denom, class_w)
    ones, nb = torch.ones(b, device=dev), torch.full((1,), float(b), device=dev)
    labels = torch.randint(0, c, (pool,), generator=g, device=dev)
    sample_w = torch.rand(pool, generator=g, device=dev)
    sampler = EpochSampler(pool, b, 1, 0, 8, device=dev, drop_last=False).begin_epoch(0)
    cands = {
        "clip_weights, batch form": lambda: ops.clip_weights(y, clip_u, denom, class_w),
        "clip_weights, sampler, world 8": lambda: ops.clip_weights(labels, clip_u, denom, class_w, sample_w, perm=sampler.perm, cursor=sampler.cursor,
                                                                 rank=3, world=8),
        "cls_head_loss": lambda: E.cls_head_loss(z, w, bias, y, 1, 0.0, None, dw, db),
        "cls_head_loss_w": lambda: E.cls_head_loss_w(z, w, bias, y, 1, 0.0, None, ones, nb, dw, db),
        "cls_head_loss_cw": lambda: E.cls_head_loss_cw(z, w, bias, y, 1, 0.0, None, clip_u, denom, dw, db),
        "ce_logits": lambda: E.ce_logits(lg, y),
        "ce_logits_w": lambda: E.ce_logits_w(lg, y, ones, nb),
        "ce_logits_cw": lambda: E.ce_logits_cw(lg, y, clip_u, denom),
    }
    for fn in cands.values():
        events(torch, fn, 10)
    got = {name: [] for name in cands}
    for _ in range(opt.rounds):
        for name, fn in cands.items():
            got[name].append(events(torch, fn, opt.launches) * 1e3)
    det = (torch.rand(pool, generator=g, device=dev) < 0.05).float()
    samplers = {"EpochSampler": EpochSampler(pool, b, 1, 0, 1, device=dev),
                "BalancedEpochSampler (redraw)": BalancedEpochSampler(det, b, 1, rank=0, world=1),
                "BalancedEpochSampler (no redraw)": BalancedEpochSampler(det, b, 1, redraw=False, rank=0, world=1)}

    def epochs(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(opt.epochs):
            s.begin_epoch(e)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / opt.epochs

    for s in samplers.values():
        epochs(s)
    ep = {name: [] for name in samplers}
    for _ in range(opt.rounds):
        for name, s in samplers.items():
            ep[name].append(epochs(s))
    print(json.dumps({"us": {k: spread(v) for k, v in got.items()}, "epoch_ms": {k: spread(v) for k, v in ep.items()},
                      "epoch_len": samplers["BalancedEpochSampler (redraw)"].epoch_len}))


if opt.step == "steps":
    step_steps()
elif opt.step == "ops":
    step_ops()
else:
    driver()
