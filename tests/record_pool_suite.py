"""Checks of clips cut out of device-resident recordings through a device clip table (eeg_gnn_ssl_amd/device_data.py:
`RecordingDataset`, the three `clip_table_*` builders; csrc/kernels_records.h: `ops.gather_records`).  As in device_epoch_suite.py the
same functions run on the GPU library and on the emulator build of the same kernel sources (tests/test_record_pool.py).

Every comparison is bit for bit (`torch.equal` / `np.array_equal`): the gather is a copy with zero fill, and the steps behind it are
the same kernels on the same inputs in the same order.  The reference result of a cut is numpy slicing written as the reference
writes it -- `signal_array[:, start:end]`, then the `while` loop over whole steps (data/dataloader_ssl.py:52-73,
dataloader_classification.py:61-81) -- zero-padded to the batch row.  Where a clip runs past the end of its recording numpy
truncates the slice; the gather's rule keeps the steps that x_samples names and fills what is not there with zeros, so the slice is
zero-filled to its nominal width BEFORE the loop (a table that wants the reference's shorter clip says so in x_samples).

Each check FAILS ON THE PARENT COMMIT: `ops.gather_records`, `RecordingDataset` and the table builders do not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from device_epoch_suite import SEED, _expected_index, _same_state
from oracle import dcrnn_oracle as orc
from parity_suite import load, make_args

N = 19
GATHER_LENGTHS = (2600, 1803, 9000)          # 1803: the stride of recording 1 is padded to 1804
B, T, W, TY, P = 4, 4, 200, 2, 10            # the step checks: three steps of 4 clips out of 10
STEP_LENGTHS = (4100, 1803, 5000)            # 20.5 s, 9 s and 25 s at 200 Hz


def _recordings(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, n, generator=g) for n in lengths]


# ---- the reference cut -------------------------------------------------------------------------------------------------------------
def _slice(sig, start, count):
    """`signal_array[:, start:start + count]` as `count` columns: numpy truncates the slice at the end of the recording (the columns
    behind it stay zero, the padding of the batch row); samples in front of the recording do not exist either"""
    out = np.zeros((sig.shape[0], max(count, 0)), dtype=np.float32)
    lo, hi = max(start, 0), min(start + count, sig.shape[1])
    if hi > lo:
        out[:, lo - start:hi - start] = sig[:, lo:hi]
    return out


def cut_reference(recs, row, window, x_steps, y_steps):
    """one table row -> (x (N, x_steps*window), whole steps, y (N, y_steps*window)) by slicing plus the reference's `while` loop;
    rec is clamped into the recordings and x_samples into 0..x_len, the rule of the kernel for entries a validated table never holds"""
    rec, x_start, x_samples, y_start = (int(v) for v in row)
    sig = recs[min(max(rec, 0), len(recs) - 1)]
    x_len = x_steps * window
    curr_slc = _slice(sig, x_start, min(max(x_samples, 0), x_len))
    start_time_step, time_steps = 0, []
    while start_time_step <= curr_slc.shape[1] - window:
        end_time_step = start_time_step + window
        time_steps.append(curr_slc[:, start_time_step:end_time_step])
        start_time_step = end_time_step
    x = np.zeros((sig.shape[0], x_len), dtype=np.float32)
    if time_steps:
        x[:, :len(time_steps) * window] = np.concatenate(time_steps, axis=1)
    return x, len(time_steps), _slice(sig, y_start, y_steps * window)


def cut_pools(recs, table, window, x_steps, y_steps):
    """the pre-cut pools of a table: x (P, N, x_len), lengths (P,), y (P, N, y_len)"""
    np_recs = [r.numpy() for r in recs]
    cuts = [cut_reference(np_recs, row, window, x_steps, y_steps) for row in np.asarray(table)]
    return (torch.from_numpy(np.stack([c[0] for c in cuts])), torch.tensor([c[1] for c in cuts], dtype=torch.int64),
            torch.from_numpy(np.stack([c[2] for c in cuts])))


# ---- 1. the gather -----------------------------------------------------------------------------------------------------------------
# (rec, x_start, x_samples, y_start) over recordings of 2600, 1803 and 9000 samples
TABLE_WIDE = np.array([                      # window 200, Tx 21 (4200 floats per channel: two block stretches), Ty 3
    (2, 0, 4200, 4200),                      # starts = 0, 1, 2, 3 mod 4 (offsets and strides are multiples of 4)
    (2, 1, 4200, 4201),
    (2, 402, 4200, 802),
    (2, 1203, 4200, 7),
    (0, 400, 4200, 0),                       # runs past the end of recording 0: zero fill
    (1, 1001, 4200, 1500),                   # ... of the padded recording, from an odd start; y crosses the end, too
    (2, 3000, 700, 8700),                    # 3.5 windows: length 3, the half step zero; y crosses the recording's end
    (2, 5, 100000, 100),                     # x_samples larger than x_len
    (0, 2400, 200, 2500),                    # the last whole step of a recording
    (1, 0, 1803, 4),
    (2, 4796, 4200, 8999),                   # y: one sample left
    (0, 1999, 601, 1),
], dtype=np.int64)
TABLE_SMALL = np.array([                     # window 8, Tx 4 (32 floats per channel), no target
    (0, 0, 32, 0), (0, 1, 32, 0), (1, 2, 32, 0), (2, 3, 32, 0), (1, 1790, 32, 0), (2, 8990, 32, 0), (2, 100, 28, 0), (0, 17, 1000, 0),
    (1, 1795, 8, 0), (0, 2587, 13, 0), (2, 4444, 9, 0), (1, 901, 31, 0),
], dtype=np.int64)


def _nan(*shape, device):
    return torch.full(shape, float("nan"), device=device)


def check_gather(device):
    """`ops.gather_records` against the reference cut of clip idx_b = clamp(perm[(cursor + rank*B + b) mod n_perm], 0, P-1): two
    geometries (docstrings of the tables), float32 and int64 labels, a shuffled perm, cursors that wrap, (rank, world) in {(0, 1),
    (1, 2)}; outputs pre-filled with NaN (an element left unwritten shows); the cursor has advanced by B*world.  Then the tail form
    at the last step of an epoch of 12 clips in steps of 5: clip_w, denom and n_valid equal those of `gather_clips_tail` on a
    sampler in the same state, and so does the batch."""
    from eeg_gnn_ssl_amd import EpochSampler, layout_recordings, ops
    recs = _recordings(GATHER_LENGTHS, 41)
    signals, rec_table = layout_recordings(recs, device)
    assert rec_table.cpu().tolist() == [[0, 2600, 2600], [19 * 2600, 1804, 1803], [19 * (2600 + 1804), 9000, 9000]]
    assert signals.numel() == 19 * (2600 + 1804 + 9000) and signals.data_ptr() % 16 == 0
    assert bool((signals[19 * 2600:19 * 4404].view(19, 1804)[:, 1803] == 0).all())             # the padding is zero
    g = torch.Generator().manual_seed(42)
    cases = 0
    for table, window, tx, ty in ((TABLE_WIDE, 200, 21, 3), (TABLE_SMALL, 8, 4, 0)):
        p, b = len(table), 4
        x_pool, len_pool, y_pool = cut_pools(recs, table, window, tx, ty)
        assert sorted(set(len_pool.tolist())) == ([1, 3, 9, 21] if ty else [1, 3, 4])
        perm = torch.randperm(p, generator=g)
        labels = (torch.rand(p, generator=g), torch.randint(0, 4, (p,), generator=g))
        clip_table = torch.from_numpy(table).to(device)
        for lab in labels:
            for rank, world, c0 in ((0, 1, 0), (0, 1, p - 3), (1, 2, 0), (1, 2, 7)):
                idx = _expected_index(perm, c0, rank, world, b, p)
                cursor = torch.tensor([c0], dtype=torch.int64, device=device)
                x_out, y_out = _nan(b, N, tx * window, device=device), (_nan(b, N, ty * window, device=device) if ty else None)
                l_out, n_out = torch.full((b,), -7, dtype=lab.dtype, device=device), torch.full((b,), -7, dtype=torch.int64, device=device)
                ops.gather_records(signals, rec_table, clip_table, x_out, perm.to(device), cursor, rank, world, window=window, y_out=y_out,
                                   label_pool=lab.to(device), label_out=l_out, len_out=n_out)
                tag = (window, str(lab.dtype), rank, world, c0)
                assert torch.equal(x_out.cpu(), x_pool[idx]), tag
                assert not ty or torch.equal(y_out.cpu(), y_pool[idx]), tag
                assert torch.equal(n_out.cpu(), len_pool[idx]) and torch.equal(l_out.cpu(), lab[idx]), tag
                assert int(cursor.item()) == c0 + b * world, tag
                cases += 1
    assert cases == 16
    # the tail form: 12 clips in steps of 5, the last step holds 2
    x_pool, len_pool, y_pool = cut_pools(recs, TABLE_WIDE, 200, 21, 3)
    rec_s = EpochSampler(12, 5, SEED, 0, 1, device=device, drop_last=False).begin_epoch(1).seek(10)
    cut_s = EpochSampler(12, 5, SEED, 0, 1, device=device, drop_last=False).begin_epoch(1).seek(10)
    for s in (rec_s, cut_s):
        s.clip_w.fill_(-1), s.denom.fill_(-1), s.n_valid.fill_(-1)
    x_out, y_out, n_out = _nan(5, N, 4200, device=device), _nan(5, N, 600, device=device), torch.zeros(5, dtype=torch.int64, device=device)
    ops.gather_records(signals, rec_table, torch.from_numpy(TABLE_WIDE).to(device), x_out, rec_s.perm, rec_s.cursor, 0, 1, window=200, y_out=y_out,
                       len_out=n_out, clip_w=rec_s.clip_w, denom=rec_s.denom, n_valid=rec_s.n_valid)
    x_cut, y_cut, n_cut = torch.empty_like(x_out), torch.empty_like(y_out), torch.empty_like(n_out)
    ops.gather_clips(x_pool.to(device), x_cut, cut_s.perm, cut_s.cursor, 0, 1, y_pool=y_pool.to(device), y_out=y_cut, len_pool=len_pool.to(device),
                     len_out=n_cut, clip_w=cut_s.clip_w, denom=cut_s.denom, n_valid=cut_s.n_valid)
    assert rec_s.clip_w.tolist() == cut_s.clip_w.tolist() == [1, 1, 0, 0, 0]
    assert rec_s.denom.item() == cut_s.denom.item() == 2.0 and rec_s.n_valid.item() == cut_s.n_valid.item() == 2
    assert torch.equal(x_out, x_cut) and torch.equal(y_out, y_cut) and torch.equal(n_out, n_cut)
    assert int(rec_s.cursor.item()) == int(cut_s.cursor.item()) == 15


# ---- 2. hostile tables -------------------------------------------------------------------------------------------------------------
def check_hostile_tables(device, everything):
    """table entries that `RecordingDataset` refuses, handed to the operator directly: the result is the rule of the kernel (rec
    clamped into 0..R-1, a sample outside the recording exactly zero, a negative x_samples no step at all) and finite.
    everything=False (the GPU): only entries for which even an UNCLAMPED address would stay inside the `signals` allocation -- the
    middle recording of three with starts off by less than a neighbour's length, and the first and last recording probed with their
    own in-range numbers (a clamp that moved them shows as the wrong recording's samples) -- so a wrong clamp is a wrong value."""
    from eeg_gnn_ssl_amd import layout_recordings, ops
    recs = _recordings(GATHER_LENGTHS, 43)
    signals, rec_table = layout_recordings(recs, device)
    rows = [(1, -50, 64, -1000), (1, 1803 + 10, 64, 1790), (1, -31, 32, 1803), (1, 1800, 1 << 40, -3),
            (0, 8, 64, 8), (2, 8, 64, 8), (1, 40, -5, 40), (1, 40, -(1 << 62), 40)]
    if everything:
        rows += [(-1, 8, 64, 8), (3, 8, 64, 8), (1 << 40, 8, 64, 8), (-(1 << 62), 8, 64, 8), (1, 1 << 62, 64, -(1 << 62)),
                 (1, -(1 << 62), 64, 1 << 62), (1, (1 << 62) + 12345, 64, (1 << 63) - 1), (1, -(1 << 63), 64, -(1 << 63)),
                 (2, 8, -(1 << 63), 8), (0, 8, (1 << 63) - 1, 8)]
    table = np.array(rows, dtype=np.int64)
    p, window, tx, ty = len(table), 8, 8, 4
    x_pool, len_pool, y_pool = cut_pools(recs, table, window, tx, ty)
    assert len_pool[:8].tolist() == [8, 8, 4, 8, 8, 8, 0, 0]       # (the length is that of x_samples, wherever the clip lies)
    perm, cursor = torch.arange(p, device=device), torch.zeros(1, dtype=torch.int64, device=device)
    x_out, y_out, n_out = _nan(p, N, tx * window, device=device), _nan(p, N, ty * window, device=device), torch.full((p,), -7, device=device)
    ops.gather_records(signals, rec_table, torch.from_numpy(table).to(device), x_out, perm, cursor, window=window, y_out=y_out, len_out=n_out)
    assert bool(torch.isfinite(x_out).all()) and bool(torch.isfinite(y_out).all())
    for i, row in enumerate(rows):
        assert torch.equal(x_out[i].cpu(), x_pool[i]) and torch.equal(y_out[i].cpu(), y_pool[i]) and int(n_out[i]) == int(len_pool[i]), row
    assert torch.equal(x_out[0, :, :50].cpu(), torch.zeros(N, 50)) and torch.equal(x_out[0, :, 50:].cpu(), recs[1][:, :14])
    assert torch.equal(x_out[4].cpu(), recs[0][:, 8:72]) and torch.equal(x_out[5].cpu(), recs[2][:, 8:72])


# ---- 3. a step from recordings equals the step from pre-cut pools ---------------------------------------------------------------------
SEIZURES = (                                 # (start_s, end_s) of every seizure of the three recordings of the step checks
    [(3.0, 5.5), (5.6, 9.1), (12.0, 20.0)],
    [(2.5, 4.2), (6.0, 8.9)],
    [(1.0, 3.0), (3.004, 6.0), (10.0, 11.3), (15.0, 22.0), (23.0, 25.0)],
)


def step_tables():
    """the clip tables of the step checks, P = 10 each, from the three builders"""
    from eeg_gnn_ssl_amd import clip_table_classification, clip_table_detection, clip_table_ssl
    det = np.concatenate([clip_table_detection([0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 4, 0, 1, 0, 2, 5], T),
                          np.array([(2, 500, T * W, 0), (0, 1303, T * W, 0)], dtype=np.int64)])     # two overlapping clips, one from an odd start
    ssl = clip_table_ssl([0, 0, 0, 0, 1, 2, 2, 2, 2, 2], [0, 1, 2, 3, 0, 0, 1, 2, 3, 4], [1, 2, 3, 4, 1, 1, 2, 3, 4, 5], T)
    rec_ids = [0, 0, 0, 1, 1, 2, 2, 2, 2, 2]
    cls = clip_table_classification(rec_ids, [SEIZURES[r] for r in rec_ids], [0, 1, 2, 0, 1, 0, 1, 2, 3, 4], T)
    return {"detection": det, "ssl": ssl, "classification": cls}


def _step_case(kind, adj3d, device, units):
    """-> (make(): a fresh (model, TrainStep) with the same initial parameters and generator seeds, RecordingDataset, the DeviceDataset
    of the same clips pre-cut with numpy, supports).  kind: detection (raw, supports=None), detection_shared (the 2-D distance graph),
    classification (padding_val=0.0, variable lengths; the pre-cut pool is zero-padded and has a seq_lengths pool), ssl (raw pairs,
    data_augment=True), timedomain (use_fft=False detection)."""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, DCRNNModel_nextTimePred, DeviceDataset, RecordingDataset, utils
    from eeg_gnn_ssl_amd.train_step import TrainStep
    recs = _recordings(STEP_LENGTHS, 44)
    g = torch.Generator().manual_seed(45)
    task = {"detection_shared": "detection", "timedomain": "detection"}.get(kind, kind)
    table = step_tables()[task]
    assert table.shape == (P, 4)
    x_pool, len_pool, y_pool = cut_pools(recs, table, W, T, TY if task == "ssl" else 0)
    supports, kw, din = None, dict(raw_window=W, raw_mean=0.3, raw_std=1.7), W // 2
    if task == "detection":
        y = torch.randint(0, 2, (P,), generator=g).float().to(device)
        assert len_pool.tolist() == [T] * P
        pools = DeviceDataset(x_pool.to(device), y)
        if kind == "detection_shared":
            supports = [s.to(device) for s in utils.compute_supports(adj3d, "laplacian")]
        if kind == "timedomain":
            kw, din = dict(kw, use_fft=False), W
    elif task == "classification":
        y = torch.randint(0, 4, (P,), generator=g).to(device)
        assert sorted(set(len_pool.tolist())) == [2, 3, 4] and any(int(s) % 4 for s in table[:, 1])
        pools = DeviceDataset(x_pool.to(device), y, len_pool.to(device))
        kw = dict(kw, padding_val=0.0)
    else:
        y = None
        pools = DeviceDataset(x_pool.to(device), y_pool.to(device))
        kw = dict(kw, data_augment=True)
    ds = RecordingDataset(recs, table, y, window=W, x_steps=T, y_steps=TY if task == "ssl" else 0, device=device)
    classes = {"detection": 1, "classification": 4, "ssl": 1}[task]
    cfg = orc.DCRNNConfig(filter_type="laplacian" if supports is not None else "dual_random_walk", input_dim=din, output_dim=din,
                          num_classes=classes, rnn_units=units)
    params = orc.init_params(cfg, "ssl" if task == "ssl" else "classification", seed=6)

    def make():
        model = DCRNNModel_nextTimePred(make_args(cfg), device=device) if task == "ssl" else DCRNNModel_classification(make_args(cfg), classes, device=device)
        load(model, params, device)
        model.train()
        torch.manual_seed(99)                                       # the seed of the step's augmentation generator
        return model, TrainStep(model, task=task, **kw)

    return make, ds, pools, supports


def _run_steps(st, data, sampler, supports, steps=3):
    """`steps` step_from calls; a sampler at the end of its epoch begins the next one"""
    losses, epoch = [], 0
    st.begin_epoch(0, 4, sampler=sampler)
    for _ in range(steps):
        if int(sampler.cursor.item()) >= sampler.steps_per_epoch * sampler.batch_size * sampler.world:
            epoch += 1
            st.begin_epoch(epoch, 4)
        losses.append(st.step_from(data, sampler, supports).clone())
    return losses


def check_step(device, adj3d, kind, drop_last, units=64):
    """three `step_from` calls on a `RecordingDataset` and on the `DeviceDataset` of the same clips cut with numpy, twins with the same
    parameters, generator seeds and sampler seed: identical losses, parameters and Adam moments.  drop_last=True: two steps of epoch
    0 and, behind `begin_epoch`, one of epoch 1; drop_last=False: the whole epoch, the third step on the 2 clips that remain."""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, pools, supports = _step_case(kind, adj3d, device, units)
    (_, a), (_, b) = make(), make()
    s_a, s_b = (EpochSampler(P, B, SEED, 0, 1, device=device, drop_last=drop_last) for _ in range(2))
    assert s_a.steps_per_epoch == (2 if drop_last else 3) and ds.has_lengths and len(ds) == P
    la, lb = _run_steps(a, ds, s_a, supports), _run_steps(b, pools, s_b, supports)
    print(f"step_from recordings {kind} drop_last={drop_last}: losses {[float(v) for v in la]}")
    for k, (u, v) in enumerate(zip(la, lb)):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all()), (kind, k, u.item(), v.item())
    assert len({float(v) for v in la}) == 3
    assert torch.equal(s_a.perm, s_b.perm) and int(s_a.cursor.item()) == int(s_b.cursor.item())
    assert a.samples_seen == b.samples_seen == (3 * B if drop_last else P)
    _same_state(a, b, f"recordings vs pools ({kind}, drop_last={drop_last})")
    if kind == "ssl":
        assert torch.equal(a.last_augmentation[0], b.last_augmentation[0])


def check_captured_epoch(device, adj3d):
    """GPU only: `capture_epoch` on a `RecordingDataset` + `replay_step` over two epochs with `begin_epoch` between them equals the
    eager `step_from` run (losses, parameters, moments); the addresses of the signal buffer and the tables do not change"""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, _, supports = _step_case("detection", adj3d, device, 64)
    (_, eager) = make()
    s_e = EpochSampler(P, B, SEED, 0, 1, device=device)
    want = []
    for e in range(2):
        eager.begin_epoch(e, 2, sampler=s_e)
        want += [eager.step_from(ds, s_e, supports).clone() for _ in range(s_e.steps_per_epoch)]
    (_, st) = make()
    s_c = EpochSampler(P, B, SEED, 0, 1, device=device).begin_epoch(0)
    keep = st.snapshot()
    st.capture_epoch(ds, s_c, supports)
    assert int(s_c.cursor.item()) == 0
    st.restore(keep)
    addrs = lambda: [t.data_ptr() for t in (ds.signals, ds.rec_table, ds.clip_table, s_c.perm, s_c.cursor)]     # noqa: E731
    addr0, got = addrs(), []
    for e in range(2):
        st.begin_epoch(e, 2)
        got += [st.replay_step().clone() for _ in range(s_c.steps_per_epoch)]
    assert addrs() == addr0 and len(got) == len(want) == 4
    for k, (u, v) in enumerate(zip(got, want)):
        assert torch.equal(u, v), (k, u.item(), v.item())
    _same_state(st, eager, "captured epoch from recordings")


# ---- 4. evaluators -----------------------------------------------------------------------------------------------------------------
def check_evaluators(device, adj3d, units=64):
    """`TrainStep.evaluator` over a `RecordingDataset` (P = 10, B = 4: a short last step) against the same over the pre-cut pools:
    identical record words, probs and losses (classification, variable lengths); `TrainStep.ssl_evaluator` likewise: clip_mae and
    the loss.  Captured passes on the GPU, eager ones on the emulator (no HIP graphs there)."""
    capture = device != "cpu"
    make, ds, pools, supports = _step_case("classification", adj3d, device, units)
    (_, st) = make()
    ev_r, ev_p = st.evaluator(ds, B, supports), st.evaluator(pools, B, supports)
    res_r, res_p = ev_r.run(capture=capture), ev_p.run(capture=capture)
    assert torch.equal(ev_r.record, ev_p.record) and list(res_r.items()) == list(res_p.items())
    assert torch.equal(ev_r.probs, ev_p.probs) and torch.equal(ev_r.losses, ev_p.losses) and bool(torch.isfinite(ev_r.probs).all())
    assert tuple(ev_r.probs.shape) == (P, 4)
    print(f"evaluator from recordings: {dict(res_r)}")
    make, ds, pools, supports = _step_case("ssl", adj3d, device, units)
    (_, st) = make()
    ev_r, ev_p = st.ssl_evaluator(ds, B, supports), st.ssl_evaluator(pools, B, supports)
    loss_r, loss_p = ev_r.run(capture=capture), ev_p.run(capture=capture)
    assert loss_r == loss_p and np.isfinite(loss_r) and torch.equal(ev_r.record, ev_p.record)
    assert torch.equal(ev_r.clip_mae, ev_p.clip_mae) and bool((ev_r.clip_mae > 0).all())
    print(f"ssl_evaluator from recordings: loss {loss_r}")


# ---- 5. the table builders (host only) ---------------------------------------------------------------------------------------------
def check_builders():
    """each builder against the reference's arithmetic written out per clip"""
    from eeg_gnn_ssl_amd import clip_table_classification, clip_table_detection, clip_table_ssl
    FREQUENCY = 200
    rec_ids, clip_idx = [3, 0, 7, 7], [0, 5, 2, 11]
    for clip_len in (12, 60):
        want = []
        for r, i in zip(rec_ids, clip_idx):                          # dataloader_detection.py computeSliceMatrix
            physical_clip_len = int(FREQUENCY * clip_len)
            start_window = i * physical_clip_len
            end_window = start_window + physical_clip_len
            want.append((r, start_window, end_window - start_window, 0))
        got = clip_table_detection(rec_ids, clip_idx, clip_len)
        assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and got.tolist() == [list(w) for w in want]
    idx_y = [1, 6, 3, 12]
    want = []
    for r, i, j in zip(rec_ids, clip_idx, idx_y):                    # dataloader_ssl.py:52-58 with clip_len=self.input_len for both halves (:303-310)
        physical_clip_len = int(FREQUENCY * 12)
        want.append((r, i * physical_clip_len, physical_clip_len, j * physical_clip_len))
    assert clip_table_ssl(rec_ids, clip_idx, idx_y, 12).tolist() == [list(w) for w in want]
    assert clip_table_ssl([0], [2], [3], 60, freq=100).tolist() == [[0, 12000, 6000, 18000]]
    # classification: both arms of the max (seizure 0 of recording 2 starts at pre_seizure_end + 1 = 1, its seizure 1 -- 4 ms behind the
    # end of seizure 0 -- at the end of seizure 0 plus 1; the others at onset - 2 s) and of the min (a clip cut by clip_len, one by the
    # seizure's end)
    rec_ids = [0, 0, 0, 1, 1, 2, 2, 2, 2, 2]
    seizure_idx = [0, 1, 2, 0, 1, 0, 1, 2, 3, 4]
    want, arms = [], set()
    for r, seizure in zip(rec_ids, seizure_idx):                     # dataloader_classification.py:44-66
        offset, clip_len, seizure_times = 2, 4, SEIZURES[r]
        curr_seizure_time = seizure_times[seizure]
        pre_seizure_end = int(FREQUENCY * seizure_times[seizure - 1][1]) if seizure > 0 else 0
        start_t = max(pre_seizure_end + 1, int(FREQUENCY * (curr_seizure_time[0] - offset)))
        end_t = min(start_t + int(FREQUENCY * clip_len), int(FREQUENCY * curr_seizure_time[1]))
        arms |= {("max", start_t == pre_seizure_end + 1, seizure > 0), ("min", end_t == start_t + int(FREQUENCY * clip_len))}
        want.append((r, start_t, end_t - start_t, 0))
    got = clip_table_classification(rec_ids, [SEIZURES[r] for r in rec_ids], seizure_idx, 4)
    assert got.tolist() == [list(w) for w in want]
    assert arms == {("max", True, False), ("max", True, True), ("max", False, False), ("max", False, True), ("min", True), ("min", False)}
    assert got[:, 1].tolist() == [200, 1101, 2000, 100, 841, 1, 601, 1600, 2600, 4401]
    assert got[:, 2].tolist() == [800, 719, 800, 740, 800, 599, 599, 660, 800, 599]
    assert clip_table_classification([0], [[(10.0, 30.0)]], [0], 12, freq=100, offset_s=3).tolist() == [[0, 700, 1200, 0]]


# ---- 6. resume ---------------------------------------------------------------------------------------------------------------------
def check_resume(device, adj3d, units=64):
    """one step of an epoch, `state_dict`, a fresh TrainStep + RecordingDataset + sampler, the rest of the epoch: equal to the
    uninterrupted run"""
    from eeg_gnn_ssl_amd import EpochSampler
    make, ds, _, supports = _step_case("classification", adj3d, device, units)
    (_, whole) = make()
    s_w = EpochSampler(P, B, SEED, 0, 1, device=device, drop_last=False)
    whole.begin_epoch(1, 4, sampler=s_w)
    for _ in range(s_w.steps_per_epoch):
        whole.step_from(ds, s_w, supports)
    (m1, first) = make()
    s_1 = EpochSampler(P, B, SEED, 0, 1, device=device, drop_last=False)
    first.begin_epoch(1, 4, sampler=s_1)
    first.step_from(ds, s_1, supports)
    state, weights = first.state_dict(), {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    assert state["sampler"] == {"seed": SEED, "epoch": 1, "cursor": B}
    make2, ds2, _, _ = _step_case("classification", adj3d, device, units)
    (m2, second) = make2()
    m2.load_state_dict(weights)
    s_2 = EpochSampler(P, B, SEED + 5, 0, 1, device=device, drop_last=False)
    second.attach_sampler(s_2)
    second.load_state_dict(state)
    for _ in range(s_2.steps_per_epoch - 1):
        second.step_from(ds2, s_2, supports)
    assert int(s_2.cursor.item()) == int(s_w.cursor.item()) and second.step_count == whole.step_count == 3
    assert second.samples_seen == whole.samples_seen == P
    _same_state(second, whole, "resumed epoch from recordings")


# ---- 7. refusals and operator registration -----------------------------------------------------------------------------------------
def check_refusals(device, adj3d):
    """each refusal names the offending value: the table validation of `RecordingDataset`, the step's window and task, `batches`, the
    operator's dtypes, devices, contiguity, shapes, window % 4, x_len % window, B*world <= n_perm, 16-byte alignment and rows of
    whole pieces, and the C entry point's own"""
    from eeg_gnn_ssl_amd import DCRNNModel_classification, EpochSampler, RecordingDataset, _lib, layout_recordings, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    recs = _recordings((1000, 603), 46)
    ok = np.array([(0, 0, 800, 0), (1, 3, 800, 0), (1, 403, 200, 0)], dtype=np.int64)
    y = torch.zeros(3, device=device)
    mk = lambda table, labels=y, **kw: RecordingDataset(recs, table, labels, **dict(dict(window=200, x_steps=4, device=device), **kw))     # noqa: E731
    ds = mk(ok)
    assert len(ds) == 3 and ds.x_shape == (N, 800) and ds.y_shape == () and not ds.y_is_target and ds.has_lengths and ds.device == y.device

    def bad(row):
        t = ok.copy()
        t[1] = row
        return t
    with pytest.raises(ValueError, match=r"clip 1 names recording rec=2, there are 2"):
        mk(bad((2, 0, 800, 0)))
    with pytest.raises(ValueError, match=r"clip 1 names recording rec=-1"):
        mk(bad((-1, 0, 800, 0)))
    with pytest.raises(ValueError, match=r"clip 1 has x_samples=199, less than one step of window=200"):
        mk(bad((1, 0, 199, 0)))
    with pytest.raises(ValueError, match=r"clip 1 starts at x_start=-4"):
        mk(bad((1, -4, 800, 0)))
    with pytest.raises(ValueError, match=r"clip 1 starts at x_start=404: no whole step of 200 samples lies inside recording 1 \(603 samples\)"):
        mk(bad((1, 404, 800, 0)))
    with pytest.raises(ValueError, match=r"clip 1 has y_start=-1"):
        mk(bad((1, 0, 800, -1)), None, y_steps=2)
    with pytest.raises(ValueError, match=r"clip_table must be an integer \(P, 4\).*float64 \(3, 4\)"):
        mk(ok.astype(np.float64))
    with pytest.raises(ValueError, match=r"clip_table must be an integer \(P, 4\).*\(3, 3\)"):
        mk(ok[:, :3])
    with pytest.raises(ValueError, match=r"window=6 must be a positive multiple of 4"):
        mk(ok, window=6)
    with pytest.raises(ValueError, match=r"y_steps=2 and y=a label pool disagree"):
        mk(ok, y_steps=2)
    with pytest.raises(ValueError, match=r"y_steps=0 and y=None disagree"):
        mk(ok, None)
    with pytest.raises(ValueError, match=r"y must be the contiguous labels \(3,\).*torch.float32 \(4,\)"):
        mk(ok, torch.zeros(4, device=device))
    with pytest.raises(ValueError, match=r"recording 1 must be float32 \(N, L_r\).*\(18, 50\)"):
        RecordingDataset([recs[0], torch.zeros(18, 50)], ok, y, window=200, x_steps=4, device=device)
    with pytest.raises(ValueError, match=r"a ready signal buffer comes with rec_table="):
        RecordingDataset(ds.signals, ok, y, window=200, x_steps=4)
    with pytest.raises(ValueError, match=r"rec_table\[1\] = \(offset=19000, stride=604, samples=605\)"):
        RecordingDataset(ds.signals, ok, y, window=200, x_steps=4, rec_table=[[0, 1000, 1000], [19000, 604, 605]], num_channels=N)
    with pytest.raises(ValueError, match=r"signals is on (cpu|cuda:0), device=meta"):
        RecordingDataset(ds.signals, ok, y, window=200, x_steps=4, rec_table=ds.rec_table, num_channels=N, device="meta")
    with pytest.raises(ValueError, match=r"y must be the contiguous labels \(3,\) on (cpu|cuda:0).*on meta"):
        mk(ok, torch.zeros(3, device="meta"))
    again = RecordingDataset(ds.signals, ok[:2], y[:2], window=200, x_steps=2, rec_table=ds.rec_table, num_channels=N)     # load once, two tables
    assert again.signals.data_ptr() == ds.signals.data_ptr() and len(again) == 2 and again.x_shape == (N, 400)
    with pytest.raises(NotImplementedError, match=r"RecordingDataset.batches is not offered.*TrainStep.evaluator"):
        ds.batches(2)
    # the step
    cfg = orc.DCRNNConfig(filter_type="dual_random_walk", input_dim=100, num_classes=1, rnn_units=16)
    model = DCRNNModel_classification(make_args(cfg), 1, device=device).to(device)
    sampler = EpochSampler(3, 2, SEED, 0, 1, device=device)
    with pytest.raises(ValueError, match=r"TrainStep: a RecordingDataset yields raw signals \(B, N, 4\*200\); the step has raw_window=None"):
        TrainStep(model, task="detection").step_from(ds, sampler, None)
    with pytest.raises(ValueError, match=r"TrainStep\(raw_window=100\) and RecordingDataset\(window=200\) disagree"):
        TrainStep(model, task="detection", raw_window=100).step_from(ds, sampler, None)
    with pytest.raises(ValueError, match=r"DeviceEvaluator: TrainStep\(raw_window=100\) and RecordingDataset\(window=200\)"):
        TrainStep(model, task="detection", raw_window=100).evaluator(ds, 2)
    with pytest.raises(ValueError, match=r"TrainStep: task='detection' needs labels.*y_steps=2"):
        TrainStep(model, task="detection", raw_window=200).step_from(mk(ok, None, y_steps=2), sampler, None)
    with pytest.raises(ValueError, match=r"TrainStep: task='ssl' needs the target cut from the recordings.*y_steps=0"):
        TrainStep(model, task="ssl", raw_window=200).step_from(ds, sampler, None)
    with pytest.raises(ValueError, match=r"DeviceSSLEvaluator: task='ssl' needs the target cut.*y_steps=0"):
        TrainStep(model, task="ssl", raw_window=200).ssl_evaluator(ds, 2)
    # the operator
    signals, rec_table = layout_recordings(recs, device)
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)     # noqa: E731
    table, perm, cursor = torch.from_numpy(ok).to(device), torch.arange(3, device=device), z(1, dtype=torch.int64)
    call = lambda **k: ops.gather_records(**dict(dict(signals=signals, rec_table=rec_table, clip_table=table, x_out=z(2, N, 800), perm=perm,     # noqa: E731
                                                      cursor=cursor, window=200), **k))
    call()
    cursor.zero_()
    with pytest.raises(RuntimeError, match=r"signals: expected dtype torch.float32, got torch.float64"):
        call(signals=signals.double())
    with pytest.raises(RuntimeError, match=r"clip_table: expected dtype torch.int64, got torch.int32"):
        call(clip_table=table.int())
    with pytest.raises(RuntimeError, match=r"clip_table: tensor must be contiguous"):
        call(clip_table=z(4, 3, dtype=torch.int64).t())
    with pytest.raises(RuntimeError, match=r"clip_table must be int64 \(P, 4\).*\(3, 3\)"):
        call(clip_table=z(3, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"rec_table must be int64 \(R, 3\).*\(2, 4\)"):
        call(rec_table=z(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"signals must be a flat float32 buffer of whole 16-byte pieces, got \(30473,\)"):
        call(signals=signals[:-3])
    with pytest.raises(RuntimeError, match=r"window=6 must be a positive multiple of 4"):
        call(window=6, x_out=z(2, N, 12))
    with pytest.raises(RuntimeError, match=r"x_out must be \(B, N, Tx\*window\) with window=200, got \(2, 19, 804\)"):
        call(x_out=z(2, N, 804))
    with pytest.raises(RuntimeError, match=r"y_out must be \(2, 19, Ty\*window\) with window=200, got \(2, 18, 400\)"):
        call(y_out=z(2, 18, 400))
    with pytest.raises(RuntimeError, match=r"batch_size\*world = 4 clips per step exceed the 3 entries of perm"):
        call(world=2)
    with pytest.raises(RuntimeError, match=r"x_out at address 0x[0-9a-f]+ is not 16-byte aligned"):
        call(x_out=z(2 * N * 800 + 1)[1:].view(2, N, 800))
    with pytest.raises(RuntimeError, match=r"label_pool must be torch.float32 or torch.int64, got torch.int32"):
        call(label_pool=z(3, dtype=torch.int32), label_out=z(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"label_pool \(4,\) / label_out \(2,\) must be \(3,\) / \(2,\)"):
        call(label_pool=z(4), label_out=z(2))
    with pytest.raises(RuntimeError, match=r"len_out must be int64 \(2,\), got \(3,\)"):
        call(len_out=z(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"clip_w, denom and n_valid come together"):
        call(clip_w=z(2))
    assert int(cursor.item()) == 0                                  # no refused call moved it
    # C ABI
    lib = _lib.get_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    xo = z(2, N, 800)
    base = dict(signals=p(signals), signal_floats=signals.numel(), rec_table=p(rec_table), R=2, clip_table=p(table), P=3, label_pool=None,
                label_out=None, label_bytes=0, perm=p(perm), n_perm=3, cursor=p(cursor), B=2, rank=0, world=1, N=N, window=200, x_len=800,
                y_len=0, x_out=p(xo), y_out=None, len_out=None, clip_w=None, denom=None, n_valid=None, stream=None)

    def refused(text, **k):
        rc = lib.query("eeg_dcrnn_gather_records", *dict(base, **k).values())
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())
    refused("null signals / rec_table / clip_table", signals=None)
    refused("null x_out", x_out=None)
    refused("null perm / cursor", cursor=None)
    refused("y_out and y_len=400 disagree", y_len=400)
    refused("label_bytes=4 disagree", label_bytes=4)
    refused("clip_w, denom and n_valid come together", clip_w=p(z(2)))
    refused("R=0 recordings", R=0)
    refused("exceed the 3 entries of perm", world=2)
    refused("window=6 unsupported", window=6)
    refused("x_len=900 unsupported", x_len=900)
    refused("signal_floats=30474 unsupported", signal_floats=signals.numel() - 2)
    refused("16-byte aligned", x_out=ctypes.c_void_p(xo.data_ptr() + 4))
    refused("must not alias the signal buffer", x_out=p(signals))
    refused("N=0 channels", N=0)
    assert int(cursor.item()) == 0


def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on both operators"""
    from eeg_gnn_ssl_amd import layout_recordings
    E = torch.ops.eeg_dcrnn
    recs = _recordings((1000, 603), 47)
    signals, rec_table = layout_recordings(recs, device)
    d = lambda t: t.to(device)     # noqa: E731
    table = d(torch.tensor([(0, 0, 64, 100), (1, 3, 64, 7), (1, 403, 30, 500)], dtype=torch.int64))
    perm = d(torch.tensor([2, 0, 1]))
    cur = lambda: d(torch.tensor([1], dtype=torch.int64))     # noqa: E731
    i64, f32 = (lambda *s: d(torch.zeros(*s, dtype=torch.int64))), (lambda *s: d(torch.zeros(*s)))     # noqa: E731
    samples = [
        (E.gather_records.default, (signals, rec_table, table, None, None, perm, cur(), 0, 1, 8, f32(2, N, 64), None, None)),
        (E.gather_records.default, (signals, rec_table, table, d(torch.rand(3)), f32(2), perm, cur(), 0, 1, 8, f32(2, N, 64), f32(2, N, 16), i64(2))),
        (E.gather_records_tail.default, (signals, rec_table, table, i64(3), i64(1), perm, cur(), 1, 2, 8, f32(1, N, 32), None, i64(1), f32(1), f32(1), i64(1))),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
