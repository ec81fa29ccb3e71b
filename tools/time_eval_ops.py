"""dev aid (GPU box): wall-clock timing of one evaluation pass over a device-resident dev set (eeg_gnn_ssl_amd/evaluation.py,
csrc/kernels_eval.h), cfg2 model (detection, distance graph, T = 60), B = 256, a pool of --pool clips (default 3000: a few thousand,
no multiple of the batch).  Candidates, each a whole pass from the first launch to the score dictionary on the host:
    evaluate            `evaluate(model, ds.batches(B, supports))`: eager forwards, `.cpu()`, sklearn.  The code of the parent commit,
                        unchanged here: its number is the parent's.
    evaluator_eager     `DeviceEvaluator.run(capture=False)`
    evaluator_captured  `DeviceEvaluator.run(capture=True)` (the graph captured before the timed rounds)
and, on the scores of one pass, the reduction alone:
    eval_metrics        `ops.eval_metrics` + the copy of the record + `scores_from_record`
    cpu_sklearn         `.cpu().numpy()` of probabilities and labels + `utils.eval_dict` (what `evaluate` does behind its last batch)
both with the threshold search (is_test, dev set: `utils.thresh_max_f1` on the host side) and without.
A pass ends in a device-to-host copy, so a host clock around it measures it whole.  Fresh process, every candidate warmed, `--rounds`
rounds alternating between the candidates; median and spread (min..max) over the rounds.  The passes' results are compared before
anything is timed.
usage: python tools/time_eval_ops.py [--rounds 7] [--seed 11] [--pool 3000] [--out profiles/eval_time_ops.json]"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (workload table, synthetic batch, model arguments)
from eeg_gnn_ssl_amd import DCRNNModel_classification, DeviceDataset, ops, utils  # noqa: E402
from eeg_gnn_ssl_amd.evaluation import scores_from_record  # noqa: E402
from eeg_gnn_ssl_amd.train_step import TrainStep, evaluate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--pool", type=int, default=3000)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), "time_eval_ops.py measures on an MI355X; there is no other path"
warnings.simplefilter("ignore")
dev = "cuda"
task, filt, t_len, B, classes = bench.WORKLOADS["cfg2"]
_, _, _, hs = bench.synthetic_batch(task, filt, t_len, B, classes, seed=opt.seed)
supports = ops.collapse_shared_supports([s.to(dev) for s in hs])
g = torch.Generator(device=dev).manual_seed(opt.seed)
pool_x = torch.randn(opt.pool, t_len, 19, 100, generator=g, device=dev)
ds = DeviceDataset(pool_x, (pool_x[:, :, :, :10].mean(dim=(1, 2, 3)) > 0).float())
torch.manual_seed(opt.seed)
model = DCRNNModel_classification(bench.make_args(filt), classes, device=dev).to(dev).train()
st = TrainStep(model, task=task)
ev_eager, ev_graph = st.evaluator(ds, B, supports=supports), st.evaluator(ds, B, supports=supports)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(cands, rounds, reps=1):
    for fn in cands.values():
        for _ in range(2):
            fn()
    got = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            got[name].append(statistics.median(timed(fn) for _ in range(reps)))
    return {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in got.items()}


result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "seed": opt.seed, "pool_clips": opt.pool, "batch": B,
          "steps_per_pass": ev_graph.sampler.steps_per_epoch, "unit": "ms per pass, host clock around a pass that ends in a device-to-host copy"}
for search in (False, True):
    kw = dict(is_test=search, eval_set="dev", best_thresh=0.5)
    want = evaluate(model, ds.batches(B, supports), task=task, **kw)
    got_e, got_g = ev_eager.run(capture=False, **kw), ev_graph.run(capture=True, **kw)
    assert list(got_e.items()) == list(got_g.items()) and torch.equal(ev_eager.probs, ev_graph.probs)
    agree = {k: abs(got_g[k] - want[k]) for k in want}
    res = alternate({"evaluate": lambda: evaluate(model, ds.batches(B, supports), task=task, **kw),
                     "evaluator_eager": lambda: ev_eager.run(capture=False, **kw),
                     "evaluator_captured": lambda: ev_graph.run(capture=True, **kw)}, opt.rounds)
    probs, losses = ev_graph.probs.clone(), ev_graph.losses.clone()
    ws, rec = ops.eval_metrics_buffers(opt.pool, 1, dev)

    def on_device():
        return scores_from_record(ops.eval_metrics(probs, ds.y, losses, search, 0.5, ws, rec).cpu(), task, 0.5)

    def on_host():
        y_prob, y_true = probs.cpu().numpy(), ds.y.cpu().numpy().astype(int)
        thresh = float(utils.thresh_max_f1(y_true=y_true, y_prob=y_prob)) if search else 0.5
        return utils.eval_dict(y_pred=(y_prob > thresh).astype(int), y=y_true, y_prob=y_prob, average="binary")[0]

    a, b = on_device(), on_host()
    assert all(abs(a[k] - b[k]) <= 1e-12 for k in b), (a, b)
    red = alternate({"eval_metrics": on_device, "cpu_sklearn": on_host}, opt.rounds, reps=5)
    result["threshold_search" if search else "given_threshold"] = {
        "pass_ms": res, "reduction_ms": red, "scores": dict(got_g), "abs_difference_to_evaluate": agree,
        "captured_over_evaluate": res["evaluator_captured"]["median"] / res["evaluate"]["median"],
        "eager_over_evaluate": res["evaluator_eager"]["median"] / res["evaluate"]["median"],
        "eval_metrics_over_cpu_sklearn": red["eval_metrics"]["median"] / red["cpu_sklearn"]["median"]}
text = json.dumps(result, indent=1)
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text + "\n")
