"""dev aid (GPU box): HIP-event timing of epochs from a device-resident data set (eeg_gnn_ssl_amd/device_data.py, csrc/kernels_data.h).
  (a) `ops.gather_clips` (x + float label + int64 length per clip; its cursor launch included) against the ATen expression
      `index_select(out=)` on x, y and lengths with a ready index, for one batch of B = 256 out of a pool of 4096 clips, as features
      (256,60,19,100) and as raw signals (256,19,12000); TB/s of 2 x batch bytes (one read, one write), beside `ops.augment_features`
      on (256,60,19,100) + (256,12,19,100) in the same process as the yardstick of the project's streaming kernels.  The gather's
      cursor is zeroed once per 16 calls (an epoch of the pool), as `begin_epoch` does.
  (b) the captured cfg2-shaped step (detection, distance graph, T = 60, B = 256, optimiser tail inside the graph):
        resident inputs on this tree -- and, with --lib PATH, on ANOTHER build of the library (the parent commit's): the step itself
        is untouched, so the two must agree within their spreads;
        from the pool (`capture_epoch`; `begin_epoch` -- keys, sort, cursor -- once per 16 steps inside the timed loop);
        with a fresh pinned host batch per step: the step captured on two input sets, the host-to-device copy of batch k+1 on a side
        stream into the set the next replay reads while batch k computes (the method of bench.py's streamed-input pass).
  (c) the same captured step from a pool whose size is NO multiple of the batch (--pool minus 100 clips): the default sampler
        (drop_last=True: the unweighted criterion, the short batch dropped) against `EpochSampler(..., drop_last=False)` (the
        validity gather and the weighted criterion in every step, the epoch one step longer) -- and, with --lib PATH, the default
        sampler on the other build, the yardstick: the parent has no other step.  `begin_epoch` once per epoch inside the timed
        loop, as in (b).
Every figure: warm, `--rounds` rounds alternating between the candidates, each round ~0.1 s per candidate (steps: 40 steps); median
and spread (min..max) over the rounds.
usage: python tools/time_epoch_ops.py [--lib PATH] [--rounds 7] [--seed 11] [--out profiles/epoch_time_ops.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (workload table, synthetic batch, model arguments)
from eeg_gnn_ssl_amd import DCRNNModel_classification, DeviceDataset, EpochSampler, _lib, ops, utils  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libeeg_dcrnn_hip.so on which the resident step is timed beside this tree's")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--pool", type=int, default=4096)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = "cuda"
B, N, T, D, W, TY, POOL = 256, 19, 60, 100, 200, 12, opt.pool
EPOCH = POOL // B
here = _lib.get_lib()
other = _lib.EegDcrnnLib(opt.lib, strict=False) if opt.lib else None


def ms_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(cands, rounds, reps=None):
    """cands: {name: callable}; returns {name: (median ms, min ms, max ms)} over alternating rounds"""
    n = {}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n[name] = reps or max(5, int(100.0 / max(ms_per_call(fn, 5), 1e-3)))            # ~0.1 s per round
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(ms_per_call(fn, n[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def with_lib(lib, fn):
    def run(*a, **k):
        keep = _lib._LIB
        _lib._LIB = lib
        try:
            return fn(*a, **k)
        finally:
            _lib._LIB = keep
    return run


def stats(res):
    return {k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}


result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "seed": opt.seed, "pool_clips": POOL, "batch": B, "other_lib": opt.lib}
g = torch.Generator(device=dev).manual_seed(opt.seed)

# ---- (a) the gather against ATen ---------------------------------------------------------------------------------------------------
sampler = EpochSampler(POOL, B, opt.seed, 0, 1, device=dev).begin_epoch(0)
index = sampler.perm[:B].clone()
labels = (torch.rand(POOL, generator=g, device=dev) > 0.5).float()
lens = torch.randint(1, T + 1, (POOL,), generator=g, device=dev)
l_out, n_out = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
rng = ops.make_rng_state(dev, stream_id=2)
_, aug_perm, aug_ls, _ = ops.draw_augmentation(rng, B, utils.swap_permutation(N).to(dev))
gather = {}
for tag, shape in (("features_256x60x19x100", (T, N, D)), ("raw_256x19x12000", (N, T * W))):
    pool = torch.randn((POOL,) + shape, generator=g, device=dev)
    out = torch.empty((B,) + shape, device=dev)
    calls = {"k": 0}

    def ours(pool=pool, out=out, calls=calls):
        if calls["k"] % EPOCH == 0:
            sampler.cursor.zero_()
        calls["k"] += 1
        ops.gather_clips(pool, out, sampler.perm, sampler.cursor, label_pool=labels, label_out=l_out, len_pool=lens, len_out=n_out)

    def aten(pool=pool, out=out):
        torch.index_select(pool, 0, index, out=out)
        torch.index_select(labels, 0, index, out=l_out)
        torch.index_select(lens, 0, index, out=n_out)

    sampler.cursor.zero_()
    ours()
    want = pool[index]
    assert torch.equal(out, want) and torch.equal(l_out, labels[index]) and torch.equal(n_out, lens[index])
    calls["k"] = 0
    res = alternate({"gather_clips": ours, "aten_index_select": aten}, opt.rounds)
    nbytes = 2.0 * (out.numel() * 4 + B * 12)
    gather[tag] = {"ms": stats(res), "MB_moved": nbytes / 1e6, "TBps": {k: nbytes / (v[0] * 1e-3) / 1e12 for k, v in res.items()},
                   "gather_over_aten": res["gather_clips"][0] / res["aten_index_select"][0]}
    del pool, out, want
fx, fy = torch.randn(B, T, N, D, generator=g, device=dev), torch.randn(B, TY, N, D, generator=g, device=dev)
res = alternate({"augment_features": lambda: ops.augment_features(fx, fy, aug_perm, aug_ls, 2.0)}, opt.rounds)
nbytes = 2.0 * 4 * (fx.numel() + fy.numel())
gather["yardstick_augment_features_256x(60+12)x19x100"] = {"ms": stats(res), "MB_moved": nbytes / 1e6,
                                                           "TBps": nbytes / (res["augment_features"][0] * 1e-3) / 1e12}
result["gather"] = gather
del fx, fy
torch.cuda.empty_cache()

# ---- (b) the captured cfg2-shaped step ---------------------------------------------------------------------------------------------
task, filt, t_len, batch, classes = bench.WORKLOADS["cfg2"]
hx, hy, hl, hs = bench.synthetic_batch(task, filt, t_len, batch, classes, seed=opt.seed)
lengths, supports = hl.to(dev), [s.to(dev) for s in hs]


def stepper():
    torch.manual_seed(opt.seed)
    model = DCRNNModel_classification(bench.make_args(filt), classes, device=dev).to(dev).train()
    return TrainStep(model, task=task, lr=3e-4, weight_decay=5e-4, max_grad_norm=5.0)


def captured(st, x, y, slot=0):
    snap = st.snapshot()
    st.capture(x, y, lengths, supports, slot=slot, include_update=True)
    st.restore(snap)


cands = {}
st_res = stepper()
sets = [(hx.to(dev), hy.to(dev)), (hx.to(dev), hy.to(dev))]
captured(st_res, *sets[0], slot=0)
captured(st_res, *sets[1], slot=1)
cands["resident_inputs"] = lambda: st_res.replay_step(0)
if other is not None:
    st_other = with_lib(other, stepper)()
    xo, yo = hx.to(dev), hy.to(dev)
    with_lib(other, captured)(st_other, xo, yo)
    cands["resident_inputs_other_lib"] = with_lib(other, lambda: st_other.replay_step(0))

pool_x = torch.randn(POOL, t_len, N, D, generator=g, device=dev)
ds = DeviceDataset(pool_x, (pool_x[:, :, :, :10].mean(dim=(1, 2, 3)) > 0).float())
st_pool, s_pool = stepper(), EpochSampler(POOL, B, opt.seed, 0, 1, device=dev)
st_pool.begin_epoch(0, 1000, sampler=s_pool)
snap = st_pool.snapshot()
st_pool.capture_epoch(ds, s_pool, supports, include_update=True)
st_pool.restore(snap)
pool_calls = {"k": 0}


def from_pool():
    if pool_calls["k"] % EPOCH == 0:
        st_pool.begin_epoch((pool_calls["k"] // EPOCH) % 1000, 1000)
    pool_calls["k"] += 1
    return st_pool.replay_step(0)


cands["from_the_pool"] = from_pool

# a fresh batch per step from pinned host memory, the method of bench.py's streamed-input pass: two captured input sets, the copy of
# batch k+1 runs on a side stream into the idle set while batch k computes
pin = [t.pin_memory() for t in (hx, hy)]
side = torch.cuda.Stream()
landed, done = [torch.cuda.Event() for _ in sets], [torch.cuda.Event() for _ in sets]
for e in done:
    e.record()
state = {"k": 0}


def fetch(i):
    with torch.cuda.stream(side):
        side.wait_event(done[i])                                 # the previous contents of set i were consumed
        sets[i][0].copy_(pin[0], non_blocking=True)
        sets[i][1].copy_(pin[1], non_blocking=True)
        landed[i].record(side)


fetch(0)


def streamed():
    i = state["k"] % 2
    state["k"] += 1
    cur = torch.cuda.current_stream()
    fetch((i + 1) % 2)                                           # the next batch travels while this step computes
    cur.wait_event(landed[i])
    out = st_res.replay_step(i)
    done[i].record(cur)
    return out


cands["pinned_host_batch_per_step"] = streamed
res = alternate(cands, opt.rounds, reps=40)
step = {"ms": stats(res), "k_clips_per_s": {k: B / v[0] for k, v in res.items()},
        "host_bytes_per_step": int(hx.numel() * 4 + hy.numel() * hy.element_size()),
        "pool_minus_resident_ms": res["from_the_pool"][0] - res["resident_inputs"][0],
        "pool_over_pinned_host": res["from_the_pool"][0] / res["pinned_host_batch_per_step"][0]}
if other is not None:
    a, o = res["resident_inputs"], res["resident_inputs_other_lib"]
    step["resident_median_within_other_libs_range"] = bool(o[1] <= a[0] <= o[2])          # the criterion: plain min..max of the other
    step["resident_median_within_other_libs_range_widened_by_own_spread"] = bool(o[1] - (a[2] - a[1]) <= a[0] <= o[2] + (a[2] - a[1]))
result["captured_cfg2_step"] = step

# ---- (c) the epoch's short last batch: drop_last=True against drop_last=False ------------------------------------------------------
POOL_ODD = POOL - 100
assert POOL_ODD % B != 0 and POOL_ODD >= B
ds_odd = DeviceDataset(pool_x[:POOL_ODD], ds.y[:POOL_ODD].contiguous())


def epoch_stepper(drop_last, lib=None):
    wrap = (lambda f: f) if lib is None else (lambda f: with_lib(lib, f))
    st, sm = wrap(stepper)(), EpochSampler(POOL_ODD, B, opt.seed, 0, 1, device=dev, drop_last=drop_last)

    def prepare():
        st.begin_epoch(0, 1000, sampler=sm)
        keep = st.snapshot()
        st.capture_epoch(ds_odd, sm, supports, include_update=True)
        st.restore(keep)
    wrap(prepare)()
    calls = {"k": 0}

    def run():
        if calls["k"] % sm.steps_per_epoch == 0:
            st.begin_epoch((calls["k"] // sm.steps_per_epoch) % 1000, 1000)
        calls["k"] += 1
        return st.replay_step(0)
    return wrap(run), sm


cands, samplers = {}, {}
for name, drop_last, lib in (("drop_last_true", True, None), ("drop_last_false", False, None), ("drop_last_true_other_lib", True, other)):
    if name.endswith("other_lib") and other is None:
        continue
    cands[name], samplers[name] = epoch_stepper(drop_last, lib)
res = alternate(cands, opt.rounds, reps=40)
tail = {"pool_clips": POOL_ODD, "steps_per_epoch": {k: v.steps_per_epoch for k, v in samplers.items()}, "ms": stats(res)}
if other is not None:
    o = res["drop_last_true_other_lib"]
    tail["other_lib_spread_ms"] = o[2] - o[1]
    for k in ("drop_last_true", "drop_last_false"):
        tail[f"{k}_minus_other_lib_ms"] = res[k][0] - o[0]
        tail[f"{k}_slower_than_other_lib_by_more_than_its_spread"] = bool(res[k][0] - o[0] > o[2] - o[1])
result["short_last_batch_cfg2_step"] = tail
torch.cuda.synchronize()
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
