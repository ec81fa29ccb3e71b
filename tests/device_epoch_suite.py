"""Checks of epochs from a device-resident data set (eeg_gnn_ssl_amd/device_data.py, csrc/kernels_data.h): the batch gather through the
device-resident permutation and cursor (`ops.gather_clips`), the epoch's shuffle (`ops.epoch_keys` + a stable sort), `DeviceDataset` /
`EpochSampler`, and `TrainStep.step_from` / `capture_epoch` / `begin_epoch` / checkpointing.  As in varlen_suite.py the same functions
run on the GPU library and on the emulator build of the same kernel sources (tests/test_device_epoch.py).

Every comparison is bit for bit (`torch.equal`): the gather is a copy, and the steps behind it are the same kernels on the same
inputs in the same order (tests/test_gpu_determinism.py shows those reproduce).

Each check FAILS ON THE PARENT COMMIT: `ops.gather_clips`, `ops.epoch_keys`, `DeviceDataset`, `EpochSampler` and `TrainStep.step_from`
do not exist there."""
import numpy as np
import pytest
import torch

from oracle import dcrnn_oracle as orc
from parity_suite import load, make_args

P, B, T, D, W, TY = 23, 4, 3, 8, 8, 2
SEED = 20240229                   # the committed seed of the permutation checks
# the emulator's permutation of P = 23 clips for (SEED, epoch 3): the GPU must draw the same (Philox is integer arithmetic, the sort stable)
PERM_SEED_EPOCH3 = [8, 17, 11, 10, 3, 14, 4, 13, 21, 15, 7, 16, 9, 19, 5, 12, 0, 2, 20, 18, 6, 1, 22]


# ---- 1. the gather -----------------------------------------------------------------------------------------------------------------
def _expected_index(perm, cursor, rank, world, b, p):
    n = perm.numel()
    pos = [(cursor + rank * b + i) % n for i in range(b)]          # (Python's %: the non-negative residue, as the kernel's wrap)
    return perm[torch.tensor(pos)].clamp(0, p - 1)


def _guarded(shape, dtype, device):
    """a batch tensor as the middle of a buffer with one sentinel row in front and one behind -> (out, check())"""
    sentinel = -77
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), sentinel, dtype=dtype, device=device)

    def intact():
        return bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    return buf[1:-1], intact


def check_gather(device):
    """`ops.gather_clips` against `pool[idx]`, idx = clamp(perm[(cursor + rank*B + b) mod n_perm], 0, P-1): 4-D features and 3-D raw
    rows at N = 4 and 19, the SSL target as second wide tensor, float and int64 labels, int64 lengths, (rank, world) in {(0,1), (0,2),
    (1,2)}, cursors 0, 7 and n_perm - 1 (wraps) plus a negative and a huge one; the cursor has advanced by B*world; perm entries
    P + 5 and -1 read clips P - 1 and 0; rows of 16 bytes (N = 1, D = 4), of 48 bytes and of 1824 bytes (no multiples of 64), and rows
    of more than one 16-KB block stretch in both wide tensors (18240 bytes: 1140 pieces).  The batch tensors sit between sentinel
    rows that must stay untouched."""
    from eeg_gnn_ssl_amd import ops
    g = torch.Generator().manual_seed(11)
    d = lambda t: t.to(device)     # noqa: E731
    perm = torch.randperm(P, generator=g)
    labels_f, labels_i = torch.rand(P, generator=g), torch.randint(0, 4, (P,), generator=g)
    lens = torch.randint(1, T + 1, (P,), generator=g)
    shapes = []
    for n in (4, 19):
        shapes += [((T, n, D), (TY, n, D)), ((n, T * W), (n, TY * W))]
    shapes += [((1, 1, 4), None), ((1, 3, 4), (1, 1, 4)), ((19, 240), (19, 240))]
    cases = 0
    for xs, ys in shapes:
        x_pool = torch.randn((P,) + xs, generator=g)
        y_pool = None if ys is None else torch.randn((P,) + ys, generator=g)
        for (rank, world) in ((0, 1), (0, 2), (1, 2)):
            for c0 in (0, 7, P - 1, -3, 2 ** 62 + 5):
                for lab in (labels_f, labels_i, None):
                    if (c0 < 0 or c0 > P) and lab is not labels_i:
                        continue                                   # (the hostile cursors once per shape and shard)
                    idx = _expected_index(perm, c0, rank, world, B, P)
                    cursor = d(torch.tensor([c0], dtype=torch.int64))
                    x_out, x_ok = _guarded((B,) + xs, torch.float32, device)
                    y_out, y_ok = (None, lambda: True) if ys is None else _guarded((B,) + ys, torch.float32, device)
                    l_out, l_ok = (None, lambda: True) if lab is None else _guarded((B,), lab.dtype, device)
                    n_out, n_ok = _guarded((B,), torch.int64, device)
                    with_len = lab is not labels_f
                    ops.gather_clips(d(x_pool), x_out, d(perm), cursor, rank, world, y_pool=None if ys is None else d(y_pool), y_out=y_out,
                                     label_pool=None if lab is None else d(lab), label_out=l_out,
                                     len_pool=d(lens) if with_len else None, len_out=n_out if with_len else None)
                    tag = (xs, ys, rank, world, c0)
                    assert torch.equal(x_out.cpu(), x_pool[idx]), tag
                    assert ys is None or torch.equal(y_out.cpu(), y_pool[idx]), tag
                    assert lab is None or torch.equal(l_out.cpu(), lab[idx]), tag
                    assert not with_len or torch.equal(n_out.cpu(), lens[idx]), tag
                    assert int(cursor.item()) == c0 + B * world, tag
                    assert x_ok() and y_ok() and l_ok() and n_ok(), tag
                    cases += 1
    # perm entries outside the pool: clamped, deterministically -- an ordinary input (the safety contract of the kernel)
    bad = perm.clone()
    bad[0], bad[2] = P + 5, -1
    x_pool = torch.randn(P, T, 4, D, generator=g)
    x_out, x_ok = _guarded((B, T, 4, D), torch.float32, device)
    l_out = d(torch.zeros(B, dtype=torch.int64))
    cursor = d(torch.zeros(1, dtype=torch.int64))
    ops.gather_clips(d(x_pool), x_out, d(bad), cursor, label_pool=d(labels_i), label_out=l_out)
    want = torch.tensor([P - 1, int(perm[1]), 0, int(perm[3])])
    assert torch.equal(x_out.cpu(), x_pool[want]) and torch.equal(l_out.cpu(), labels_i[want]) and x_ok()
    # a perm longer than the pool (n_perm != P): the wrap runs over n_perm, the clamp over P
    long_perm = torch.cat([perm, torch.tensor([P, 2 * P])])
    cursor = d(torch.tensor([P - 1], dtype=torch.int64))
    ops.gather_clips(d(x_pool), x_out, d(long_perm), cursor)
    want = torch.tensor([int(perm[P - 1]), P - 1, P - 1, int(perm[0])])
    assert torch.equal(x_out.cpu(), x_pool[want]) and x_ok()
    assert cases > 100


# ---- 2. keys and permutation -------------------------------------------------------------------------------------------------------
def check_keys_and_permutation(device):
    """`EpochSampler.begin_epoch`: perm is a permutation of arange(P), written in place (address unchanged), cursor zeroed; equal for
    equal (seed, epoch) and independent of B, rank and world; epochs 0 and 1 differ, seeds differ; the keys lie in [0, 2^63);
    the permutation of (SEED, epoch 3) is the recorded literal (the emulator's: the GPU draws the same); spread: over 512 epochs
    with P = 8 each clip lands first between 32 and 96 times (binomial mean 64, sd 7.5: +-4 sd; the sequence is deterministic)."""
    from eeg_gnn_ssl_amd import EpochSampler, ops
    s = EpochSampler(P, B, SEED, rank=0, world=1, device=device)
    assert s.steps_per_epoch == P // B and s.epoch is None and torch.equal(s.perm.cpu(), torch.arange(P))
    addr = (s.perm.data_ptr(), s.cursor.data_ptr())
    s.cursor.fill_(9)
    s.begin_epoch(0)
    p0 = s.perm.cpu().clone()
    assert (s.perm.data_ptr(), s.cursor.data_ptr()) == addr and int(s.cursor.item()) == 0 and s.epoch == 0
    assert torch.equal(p0.sort().values, torch.arange(P))
    keys = ops.epoch_keys(torch.empty(P, dtype=torch.int64, device=device), SEED, 0).cpu()
    assert bool((keys >= 0).all()) and keys.unique().numel() == P
    assert torch.equal(torch.sort(keys, stable=True).indices, p0)
    s.begin_epoch(1)
    p1 = s.perm.cpu().clone()
    assert torch.equal(p1.sort().values, torch.arange(P)) and not torch.equal(p0, p1)
    other = EpochSampler(P, 2, SEED, rank=1, world=3, device=device).begin_epoch(0)
    assert other.steps_per_epoch == P // 6 and torch.equal(other.perm.cpu(), p0)
    assert torch.equal(EpochSampler(P, B, SEED, 0, 1, device=device).begin_epoch(1).perm.cpu(), p1)
    assert not torch.equal(EpochSampler(P, B, SEED + 1, 0, 1, device=device).begin_epoch(0).perm.cpu(), p0)
    assert s.begin_epoch(3).perm.cpu().tolist() == PERM_SEED_EPOCH3
    small = EpochSampler(8, 2, SEED, 0, 1, device=device)
    first = torch.zeros(8, dtype=torch.int64)
    for e in range(512):
        first[int(small.begin_epoch(e).perm[0].item())] += 1
    print("first-place counts over 512 epochs:", first.tolist())
    assert int(first.sum()) == 512 and 32 <= int(first.min()) and int(first.max()) <= 96, first.tolist()


# ---- 3. epoch coverage -------------------------------------------------------------------------------------------------------------
def check_epoch_coverage(device):
    """with labels = arange(P) the labels of steps_per_epoch gathers concatenate to perm[:steps*B]; ranks 0 / 1 of world 2 take
    disjoint shards whose union, step by step, is perm[:steps*2B]; `DeviceDataset.batches` yields sequential views, the last partial
    batch included, without a copy"""
    from eeg_gnn_ssl_amd import DeviceDataset, EpochSampler, ops
    g = torch.Generator().manual_seed(12)
    x = torch.randn(P, T, 4, D, generator=g).to(device)
    ds = DeviceDataset(x, torch.arange(P, dtype=torch.int64, device=device))
    x_out, y_out = torch.empty(B, T, 4, D, device=device), torch.empty(B, dtype=torch.int64, device=device)

    def epoch(sampler):
        got = []
        for _ in range(sampler.steps_per_epoch):
            ops.gather_clips(ds.x, x_out, sampler.perm, sampler.cursor, sampler.rank, sampler.world, label_pool=ds.y, label_out=y_out)
            assert torch.equal(x_out, ds.x[y_out])
            got.append(y_out.cpu().clone())
        return got

    s = EpochSampler(P, B, SEED, 0, 1, device=device).begin_epoch(2)
    assert torch.equal(torch.cat(epoch(s)), s.perm.cpu()[:s.steps_per_epoch * B]) and s.steps_per_epoch == 5
    r0 = EpochSampler(P, B, SEED, 0, 2, device=device).begin_epoch(2)
    r1 = EpochSampler(P, B, SEED, 1, 2, device=device).begin_epoch(2)
    assert r0.steps_per_epoch == r1.steps_per_epoch == 2 and torch.equal(r0.perm, r1.perm) and torch.equal(r0.perm, s.perm)
    a, b = epoch(r0), epoch(r1)
    both = torch.cat([torch.cat([u, v]) for u, v in zip(a, b)])
    assert torch.equal(both, s.perm.cpu()[:2 * 2 * B]) and both.unique().numel() == both.numel()
    assert not set(torch.cat(a).tolist()) & set(torch.cat(b).tolist())
    views = list(ds.batches(B, supports=None))
    assert [v[0].shape[0] for v in views] == [4, 4, 4, 4, 4, 3] and all(v[3] is None for v in views)
    assert views[1][0].data_ptr() == ds.x[B:].data_ptr() and torch.equal(torch.cat([v[1] for v in views]), ds.y)
    # no length pool: whole clips, the constant int64 lengths the model's last-step gather reads (T of a 4-D pool)
    assert all(v[2].dtype == torch.int64 and v[2].tolist() == [T] * v[0].shape[0] for v in views)
    lens = torch.arange(P, dtype=torch.int64, device=device) % T + 1
    with_len = list(DeviceDataset(x, ds.y, lens).batches(B))
    assert with_len[1][2].data_ptr() == lens[B:].data_ptr() and torch.equal(torch.cat([v[2] for v in with_len]), lens)
    raw = DeviceDataset(torch.zeros(P, 4, T * W, device=device), ds.y)
    assert [v[2].tolist() for v in raw.batches(B, raw_window=W)][-1] == [T] * 3
    assert all(v[2] is None for v in DeviceDataset(raw.x, torch.zeros(P, 4, TY * W, device=device)).batches(B))     # a target pool


# ---- 3b. evaluation over the pools ---------------------------------------------------------------------------------------------------
def check_evaluation_from_batches(device, adj3d, units=64):
    """`DeviceDataset.batches` feeds the existing `predict` / `evaluate` / `evaluate_ssl`: the same call on hand-sliced tensors (the
    lengths written out by hand) returns identical probabilities, labels, scores and loss.  Detection on a feature pool WITHOUT a
    length pool and the shared 2-D graph (the default form: `batches` yields the full lengths T), classification on a feature pool
    with a length pool and supports=None, ssl on a feature pair (`evaluate_ssl`, lengths None).  Last partial batch included."""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, DeviceDataset, utils
    from eeg_gnn_ssl_amd.train_step import evaluate, evaluate_ssl, predict
    g = torch.Generator().manual_seed(31)
    n = 19
    x = torch.randn(P, T, n, D, generator=g).to(device)
    spans = [(i, min(i + B, P)) for i in range(0, P, B)]
    for task, classes in (("detection", 1), ("classification", 4)):
        cfg = orc.DCRNNConfig(filter_type="laplacian" if task == "detection" else "dual_random_walk", input_dim=D, num_classes=classes,
                              rnn_units=units)
        model = DCRNNModel_classification(make_args(cfg), classes, device=device)
        load(model, orc.init_params(cfg, "classification", seed=6), device)
        if task == "detection":
            y, lens_pool = torch.randint(0, 2, (P,), generator=g).float().to(device), None
            supports = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")]
            lens = torch.full((P,), T, dtype=torch.int64, device=device)
        else:
            y, supports = torch.randint(0, 4, (P,), generator=g).to(device), None
            lens = lens_pool = torch.randint(1, T + 1, (P,), generator=g).to(device)
        ds = DeviceDataset(x, y, lens_pool)
        by_hand = [(x[i:j], y[i:j], lens[i:j], supports) for i, j in spans]
        prob, lab = predict(model, ds.batches(B, supports), task=task)
        prob_h, lab_h = predict(model, by_hand, task=task)
        assert prob.shape[0] == P and np.array_equal(prob, prob_h) and np.array_equal(lab, lab_h) and np.isfinite(prob).all(), task
        got, want = evaluate(model, ds.batches(B, supports), task=task), evaluate(model, by_hand, task=task)
        assert list(got.items()) == list(want.items()) and np.isfinite(got["loss"]), (task, got, want)
        print(f"evaluate {task} from batches: {dict(got)}")
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=D, output_dim=D, rnn_units=units)
    model = DCRNNModel_nextTimePred(make_args(cfg), device=device)
    load(model, orc.init_params(cfg, "ssl", seed=6), device)
    target = torch.randn(P, TY, n, D, generator=g).to(device)
    ds = DeviceDataset(x, target)
    got = evaluate_ssl(model, ds.batches(B), scaler_mean=0.3, scaler_std=1.7, return_predictions=True)
    want = evaluate_ssl(model, [(x[i:j], target[i:j], None) for i, j in spans], scaler_mean=0.3, scaler_std=1.7, return_predictions=True)
    assert got[0] == want[0] and np.isfinite(got[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[1].shape[0] == P
    print(f"evaluate_ssl from batches: {got[0]}")


# ---- 4. the step -------------------------------------------------------------------------------------------------------------------
def _step_case(mode, adj3d, device, units=64, manual_seed=99):
    """-> (make(): a fresh (model, TrainStep) pair with the same initial parameters and generator seeds, dataset, supports); units:
    rnn_units (64 on the GPU; the emulator leg runs 16, a front end to the step is what is checked here, not the step's kernels)"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, DeviceDataset, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    g = torch.Generator().manual_seed(21)
    n = 19
    if mode == "detection":             # features, the 2-D distance graph (spectral path)
        cfg = orc.DCRNNConfig(filter_type="laplacian", input_dim=D, num_classes=1, rnn_units=units)
        ds = DeviceDataset(torch.randn(P, T, n, D, generator=g).to(device), torch.randint(0, 2, (P,), generator=g).float().to(device))
        supports = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")]
        kind, kw, task = "classification", dict(), "detection"
    elif mode == "classification":      # raw signals, variable lengths, correlation graphs
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W // 2, num_classes=4, rnn_units=units)
        ds = DeviceDataset(torch.randn(P, n, T * W, generator=g).to(device), torch.randint(0, 4, (P,), generator=g).to(device),
                           torch.randint(1, T + 1, (P,), generator=g).to(device))
        supports, kind, task = None, "classification", "classification"
        kw = dict(raw_window=W, raw_mean=0.3, raw_std=1.7, padding_val=0.0)
    else:                               # the raw SSL pair, augmented, correlation graphs
        cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=W // 2, output_dim=W // 2, rnn_units=units)
        ds = DeviceDataset(torch.randn(P, n, T * W, generator=g).to(device), torch.randn(P, n, TY * W, generator=g).to(device))
        supports, kind, task = None, "ssl", "ssl"
        kw = dict(raw_window=W, raw_mean=0.3, raw_std=1.7, data_augment=True)
    params = orc.init_params(cfg, kind, seed=6)

    def make():
        if task == "ssl":
            model = DCRNNModel_nextTimePred(make_args(cfg), device=device)
        else:
            model = DCRNNModel_classification(make_args(cfg), cfg.num_classes, device=device)
        load(model, params, device)
        model.train()
        torch.manual_seed(manual_seed)                              # the seed of the step's augmentation generator
        return model, TrainStep(model, task=task, **kw)

    return make, ds, supports


def _state(st):
    return st.fp.flat.detach().clone(), st.exp_avg.clone(), st.exp_avg_sq.clone()


def _same_state(a, b, what):
    for name, u, v in zip(("parameters", "exp_avg", "exp_avg_sq"), _state(a), _state(b)):
        assert torch.equal(u, v), f"{what}: {name} differ by {(u - v).abs().max().item():.3e}"


def check_step_from(device, adj3d, mode, units=64):
    """`step_from` over one epoch (5 steps of B = 4 out of P = 23) and a twin `TrainStep` (same initial parameters, same generator
    seeds) fed `step(pool_x[idx], pool_y[idx], pool_len[idx], supports)` by hand with idx = perm[s*B:(s+1)*B]: identical losses,
    parameters and Adam moments.  mode: detection (features, 2-D distance graph: the spectral path), classification (raw signals,
    padding_val, supports=None), ssl (raw pair, data_augment=True, supports=None)."""
    from eeg_gnn_ssl_amd import EpochSampler, ops
    make, ds, supports = _step_case(mode, adj3d, device, units)
    (_, a), (_, b) = make(), make()
    sampler = EpochSampler(P, B, SEED, 0, 1, device=device)
    before = ops.spectral_layer_calls
    a.begin_epoch(0, 4, sampler=sampler)
    b.set_epoch(0, 4)
    perm = sampler.perm.clone()
    full = torch.full((B,), T, dtype=torch.int64, device=device)
    losses = []
    for s in range(sampler.steps_per_epoch):
        la = a.step_from(ds, sampler, supports)
        idx = perm[s * B:(s + 1) * B]
        lens = full if ds.seq_lengths is None else ds.seq_lengths[idx]
        lb = b.step(ds.x[idx], ds.y[idx], None if mode == "ssl" else lens, supports)
        assert torch.equal(la, lb), (mode, s, la.item(), lb.item())
        losses.append(float(la.item()))
    print(f"step_from {mode}: losses {losses}")
    assert int(sampler.cursor.item()) == sampler.steps_per_epoch * B and a.step_count == b.step_count == sampler.steps_per_epoch
    assert a.samples_seen == b.samples_seen == sampler.steps_per_epoch * B
    assert len(set(losses)) == len(losses) and all(np.isfinite(losses))      # (other clips every step)
    _same_state(a, b, f"step_from {mode}")
    if mode == "detection":
        assert ops.spectral_layer_calls > before, "the shared 2-D graph takes the spectral form"
    if mode == "ssl":
        assert torch.equal(a.last_augmentation[0], b.last_augmentation[0]) and a._augment_rng[1].item() == b._augment_rng[1].item() > 0


def check_captured_epoch(device, adj3d):
    """GPU only: `capture_epoch` + `replay_step` over two epochs with `begin_epoch` between them equals the eager `step_from` run
    (losses, parameters, moments) -- with the optimiser tail outside the graph and inside it; the addresses of the pools, of the
    graph's static inputs and of perm / cursor do not change."""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, supports = _step_case("detection", adj3d, device)
    (_, eager) = make()
    s_e = EpochSampler(P, B, SEED, 0, 1, device=device)
    want = []
    for e in range(2):
        eager.begin_epoch(e, 2, sampler=s_e)
        want += [eager.step_from(ds, s_e, supports).clone() for _ in range(s_e.steps_per_epoch)]
    for include_update in (False, True):
        (_, st) = make()
        s_c = EpochSampler(P, B, SEED, 0, 1, device=device)
        s_c.begin_epoch(0)
        s_c.cursor.fill_(8)
        keep = st.snapshot()
        st.capture_epoch(ds, s_c, supports, include_update=include_update)
        assert int(s_c.cursor.item()) == 8                        # the warm-up gathers moved it; it is back
        st.restore(keep)
        inputs = st._graphs[0][2]
        addrs = lambda: [t.data_ptr() for t in (ds.x, ds.y, inputs[0], inputs[1], inputs[2], s_c.perm, s_c.cursor)]     # noqa: E731
        addr0 = addrs()
        got = []
        for e in range(2):
            st.begin_epoch(e, 2)
            for k in range(s_c.steps_per_epoch):
                got.append(st.replay_step().clone())
                assert int(s_c.cursor.item()) == (k + 1) * B
        assert addrs() == addr0
        for k, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(u, v), (include_update, k, u.item(), v.item())
        assert st.step_count == eager.step_count == 2 * s_c.steps_per_epoch and st.samples_seen == eager.samples_seen
        _same_state(st, eager, f"captured epoch (include_update={include_update})")


# ---- 5. resume ---------------------------------------------------------------------------------------------------------------------
def check_resume(device, adj3d, units=64):
    """two steps of an epoch, `state_dict` (it carries the sampler's seed, epoch and cursor; the existing keys are unchanged), loaded
    into a fresh TrainStep + sampler: finishing the epoch gives the parameters of the uninterrupted run"""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, supports = _step_case("detection", adj3d, device, units)
    (_, whole) = make()
    s_w = EpochSampler(P, B, SEED, 0, 1, device=device)
    whole.begin_epoch(1, 4, sampler=s_w)
    for _ in range(s_w.steps_per_epoch):
        whole.step_from(ds, s_w, supports)
    (m1, first) = make()
    assert set(first.state_dict()) == {"step", "samples_seen", "lr", "exp_avg", "exp_avg_sq"}     # no sampler attached: as before
    s_1 = EpochSampler(P, B, SEED, 0, 1, device=device)
    first.begin_epoch(1, 4, sampler=s_1)
    for _ in range(2):
        first.step_from(ds, s_1, supports)
    state, weights = first.state_dict(), {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    assert state["sampler"] == {"seed": SEED, "epoch": 1, "cursor": 2 * B}
    assert set(state) == {"step", "samples_seen", "lr", "exp_avg", "exp_avg_sq", "sampler"}
    (m2, second) = make()
    m2.load_state_dict(weights)
    s_2 = EpochSampler(P, B, SEED + 5, 0, 1, device=device)       # (another seed: the checkpoint's takes over)
    second.attach_sampler(s_2)
    second.load_state_dict(state)
    assert s_2.state_dict() == state["sampler"] and torch.equal(s_2.perm, s_1.perm)
    for _ in range(s_2.steps_per_epoch - 2):
        second.step_from(ds, s_2, supports)
    assert int(s_2.cursor.item()) == int(s_w.cursor.item()) and second.step_count == whole.step_count
    _same_state(second, whole, "resumed epoch")
    # the other order: the checkpoint is loaded BEFORE any sampler is attached -- its sampler state is kept and applied to the first
    # sampler attached (here by step_from), never dropped
    (m3, third) = make()
    m3.load_state_dict(weights)
    third.load_state_dict(state)
    assert third.sampler is None and "sampler" not in third.state_dict()
    s_3 = EpochSampler(P, B, SEED + 7, 0, 1, device=device)
    third.step_from(ds, s_3, supports)
    assert s_3.seed == SEED and s_3.epoch == 1 and int(s_3.cursor.item()) == 3 * B and torch.equal(s_3.perm, s_1.perm)
    for _ in range(s_3.steps_per_epoch - 3):
        third.step_from(ds, s_3, supports)
    _same_state(third, whole, "resumed epoch (checkpoint loaded before the sampler was attached)")
    third.load_state_dict(state)                                    # a sampler is attached now: applied at once
    assert int(s_3.cursor.item()) == 2 * B


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d):
    """each refusal names the argument: pools on different devices, a non-contiguous pool, unequal leading dimensions,
    batch_size*world > P, a wide row that is no multiple of 16 bytes (host layer, operator and C entry point), padding_val without a
    length pool; the C entry point refuses null pointers, an in-place call and B*world > n_perm"""
    import ctypes
    from eeg_gnn_ssl_amd import DeviceDataset, EpochSampler, _lib, ops
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    with pytest.raises(ValueError, match=r"DeviceDataset: y is on meta"):
        DeviceDataset(z(P, T, 4, D), torch.zeros(P, device="meta"))
    with pytest.raises(ValueError, match=r"DeviceDataset: x must be contiguous"):
        DeviceDataset(z(P, 4, T, D).transpose(1, 2), z(P))
    with pytest.raises(ValueError, match=r"DeviceDataset: seq_lengths holds 22 clips, x holds 23"):
        DeviceDataset(z(P, T, 4, D), z(P), z(P - 1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"DeviceDataset: y holds 24 clips"):
        DeviceDataset(z(P, T, 4, D), z(P + 1))
    with pytest.raises(ValueError, match=r"DeviceDataset: a clip of x has 12 bytes"):
        DeviceDataset(z(P, 1, 1, 3), z(P))
    with pytest.raises(ValueError, match=r"DeviceDataset: a clip of y has 24 bytes"):
        DeviceDataset(z(P, 1, 1, 4), z(P, 1, 2, 3))
    with pytest.raises(ValueError, match=r"EpochSampler: batch_size\*world = 12\*2 clips per step, the pool holds P=23"):
        EpochSampler(P, 12, SEED, 0, 2, device=device)
    with pytest.raises(ValueError, match=r"EpochSampler: rank=2 of world=2"):
        EpochSampler(P, B, SEED, 2, 2, device=device)
    make, ds, supports = _step_case("classification", adj3d, device)
    (_, st) = make()
    no_len = DeviceDataset(ds.x, ds.y)
    with pytest.raises(ValueError, match=r"padding_val.*seq_lengths pool"):
        st.step_from(no_len, EpochSampler(P, B, SEED, 0, 1, device=device), None)
    (_, st_raw) = _step_case("detection", adj3d, device)[0]()       # no raw_window: a raw pool without lengths has no step count
    with pytest.raises(ValueError, match=r"TrainStep\(raw_window=\.\.\.\): x \(23, 19, 24\) holds raw signals.*raw_window=None"):
        st_raw.step_from(no_len, EpochSampler(P, B, SEED, 0, 1, device=device), None)
    with pytest.raises(ValueError, match=r"DeviceDataset.batches: x \(23, 19, 24\) holds raw signals.*raw_window=5"):
        next(no_len.batches(B, raw_window=5))
    with pytest.raises(ValueError, match=r"the dataset holds 23 clips, the sampler permutes P=20"):
        st.step_from(ds, EpochSampler(20, B, SEED, 0, 1, device=device), None)
    with pytest.raises(RuntimeError, match="no sampler attached"):
        make()[1].begin_epoch(0, 2)
    # the operators
    perm, cursor = torch.arange(P, device=device), z(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"a clip of x_pool has 12 bytes"):
        ops.gather_clips(z(P, 3), z(B, 3), perm, cursor)
    with pytest.raises(RuntimeError, match=r"x_pool: tensor must be contiguous"):
        ops.gather_clips(z(P, 8, 4).transpose(1, 2), z(B, 4, 8), perm, cursor)
    with pytest.raises(RuntimeError, match=r"y_pool holds 22 clips"):
        ops.gather_clips(z(P, 4), z(B, 4), perm, cursor, y_pool=z(P - 1, 4), y_out=z(B, 4))
    with pytest.raises(RuntimeError, match=r"label_pool must be torch.float32 or torch.int64"):
        ops.gather_clips(z(P, 4), z(B, 4), perm, cursor, label_pool=z(P, dtype=torch.int32), label_out=z(B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"batch_size\*world = 24 clips per step exceed the 23 entries of perm"):
        ops.gather_clips(z(P, 4), z(B, 4), perm, cursor, 0, 6)
    with pytest.raises(RuntimeError, match=r"perm: expected dtype torch.int64"):
        ops.gather_clips(z(P, 4), z(B, 4), perm.to(torch.int32), cursor)
    with pytest.raises(RuntimeError, match=r"epoch_keys: .*epoch=-1"):
        ops.epoch_keys(z(P, dtype=torch.int64), SEED, -1)
    assert int(cursor.item()) == 0                                  # no refused call moved it
    # C ABI
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    xp, xo, lp, lo = z(P, 4), z(B, 4), z(P), z(B)
    gather = lambda *a: lib.query("eeg_dcrnn_gather_clips", *a)     # noqa: E731
    refused(gather(None, p(xo), 16, None, None, 0, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 1, None), "null x_pool")
    refused(gather(p(xp), p(xo), 16, None, None, 0, None, None, 0, None, None, None, P, P, p(cursor), B, 0, 1, None), "null perm / cursor")
    refused(gather(p(xp), p(xo), 12, None, None, 0, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 1, None), "x_row_bytes=12")
    refused(gather(p(xp), p(xo), 16, p(xp), None, 16, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 1, None), "y_pool, y_out and y_row_bytes")
    refused(gather(p(xp), p(xo), 16, None, None, 0, p(lp), p(lo), 2, None, None, p(perm), P, P, p(cursor), B, 0, 1, None), "label_bytes=2")
    refused(gather(p(xp), p(xp), 16, None, None, 0, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 1, None), "in-place")
    refused(gather(p(xp), p(xo), 16, None, None, 0, None, None, 0, None, None, p(perm), P, P, p(cursor), B, 0, 6, None), "exceed the 23 entries")
    refused(gather(p(xp), p(xo), 16, None, None, 0, None, None, 0, None, None, p(perm), P, 0, p(cursor), B, 0, 1, None), "P=0 clips")
    refused(lib.query("eeg_dcrnn_epoch_keys", 1, 0, P, None, None), "epoch_keys: null output")
    refused(lib.query("eeg_dcrnn_epoch_keys", 1, 2 ** 31, P, p(perm), None), "epoch=2147483648")
    assert int(cursor.item()) == 0


# ---- 7. operator registration ------------------------------------------------------------------------------------------------------
def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on both operators"""
    E = torch.ops.eeg_dcrnn
    g = torch.Generator().manual_seed(3)
    d = lambda t: t.to(device)     # noqa: E731
    perm = d(torch.randperm(P, generator=g))
    cur = lambda: d(torch.tensor([5], dtype=torch.int64))     # noqa: E731
    i64 = lambda n: d(torch.zeros(n, dtype=torch.int64))     # noqa: E731
    samples = [
        (E.epoch_keys.default, (i64(P), SEED, 2)),
        (E.gather_clips.default, (d(torch.randn(P, T, 4, D, generator=g)), d(torch.zeros(B, T, 4, D)), None, None, None, None, None, None, perm, cur(), 0, 1)),
        (E.gather_clips.default, (d(torch.randn(P, 4, T * W, generator=g)), d(torch.zeros(B, 4, T * W)), d(torch.randn(P, 4, TY * W, generator=g)),
                                  d(torch.zeros(B, 4, TY * W)), None, None, None, None, perm, cur(), 1, 2)),
        (E.gather_clips.default, (d(torch.randn(P, T, 4, D, generator=g)), d(torch.zeros(B, T, 4, D)), None, None, d(torch.rand(P, generator=g)),
                                  d(torch.zeros(B)), d(torch.randint(1, 4, (P,), generator=g)), i64(B), perm, cur(), 0, 1)),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
