"""Checks of whole-recording scans (eeg_gnn_ssl_amd/scan.py: `Scanner`, `ScanResult`, `TrainStep.scanner`; device_data.py:
`clip_table_scan`, `clip_labels_detection`, `annotation_bins`; csrc/kernels_scan.h: `ops.scan_timeline`, `ops.scan_events`,
`ops.event_scores`).  As in scaler_fit_suite.py the same functions run on the GPU library and on the emulator build of the same kernel
sources (tests/test_scan.py).

Each check FAILS ON THE PARENT COMMIT: none of these names exists there (the module does not import).

The oracle is a direct numpy restatement of the semantics in include/eeg_dcrnn.h: float32 accumulation in the stated order for values
(one np.float32 per operation), Python integers for everything else.  Tolerances:
  timeline  the test probabilities are multiples of 2^-8 in [0, 1]: every float32 sum of fewer than 65536 of them is exact, so only the
            division rounds: within 1 ulp of the float64 mean rounded to float32, bit-equal where cover is a power of two; max and
            cover exact;
  smoothed  values in [0, 1]: one rounding of at most 2^-24 per add (partial sums below smooth_bins, but each add's error is relative
            to a sum that is at most smooth_bins; the quotient brings it back below 1) and one for the division:
            (smooth_bins + 2) * 2^-24 against the float64 oracle;
  events    integers, equal.  The oracle's float64 q of every covered bin lies at least 2^-12 from both thresholds in every case
            (asserted per case, no bin excluded), far above the bound on smoothed, so the comparison of a float32 q with a threshold
            cannot fall differently;
  the pass  bit for bit (torch.equal) against `DeviceEvaluator` over the same table and over the pools pre-cut with numpy -- the
            comparison and the tolerance (none) of record_pool_suite.check_evaluators; `evaluate` / `predict` take no raw pools, so
            they are not part of that comparison there or here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import record_pool_suite as rp

T, S_STRIDE, W = 4, 2, 200
SMALL = [3, 4, 5, 9, 14]
TH_ON, TH_OFF = 0.7, 0.3
MARGIN = 2.0 ** -12


def rec_steps(ops):
    return SMALL + [ops.SCAN_CHUNK_BINS + 3]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def oracle_timeline(probs, table, clip_off, steps, x_steps, window, agg):
    """-> (timeline float32, cover int, mean in float64) over the flat bins"""
    tl, cover, exact = [], [], []
    for r, s_r in enumerate(steps):
        first = int(clip_off[r])
        starts = np.asarray(table[first:int(clip_off[r + 1]), 1], dtype=np.int64) // window
        for j in range(s_r):
            hit = (first + np.nonzero((starts <= j) & (j < starts + x_steps))[0]).tolist()
            acc = np.float32(0.0)
            for k in hit:
                acc = np.float32(acc + np.float32(probs[k]))
            if not hit:
                val = np.float32(0.0)
            elif agg == "mean":
                val = np.float32(acc / np.float32(len(hit)))
            else:
                val = np.float32(max(float(probs[k]) for k in hit))
            tl.append(val)
            cover.append(len(hit))
            exact.append(sum(float(probs[k]) for k in hit) / len(hit) if hit else 0.0)
    return np.asarray(tl, dtype=np.float32), np.asarray(cover, dtype=np.int64), np.asarray(exact, dtype=np.float64)


def oracle_events(tl, cover, smooth_bins, th_on, th_off, merge_gap, min_bins):
    """one recording: timeline float32 (S,), cover (S,) -> (events [(a, b)], q float32, q float64, margin of the covered bins)"""
    s_r, h = len(tl), (smooth_bins - 1) // 2
    th_on, th_off = float(np.float32(th_on)), float(np.float32(th_off))
    q32, q64, margin = np.zeros(s_r, dtype=np.float32), np.zeros(s_r), math.inf
    state, states = False, []
    for j in range(s_r):
        if cover[j] > 0:
            idx = [i for i in range(max(j - h, 0), min(j + h, s_r - 1) + 1) if cover[i] > 0]
            acc = np.float32(0.0)
            for i in idx:
                acc = np.float32(acc + np.float32(tl[i]))
            q32[j] = np.float32(acc / np.float32(len(idx)))
            q64[j] = sum(float(tl[i]) for i in idx) / len(idx)
            margin = min(margin, abs(q64[j] - th_on), abs(q64[j] - th_off))
            if float(q32[j]) >= th_on:
                state = True
            elif float(q32[j]) < th_off:
                state = False
        else:
            state = False
        states.append(state)
    runs, a = [], None
    for j, on in enumerate(states + [False]):
        if on and a is None:
            a = j
        if not on and a is not None:
            runs.append((a, j))
            a = None
    merged = []
    for a, b in runs:
        if merged and a - merged[-1][1] <= merge_gap:
            merged[-1] = (merged[-1][0], b)
        else:
            merged.append((a, b))
    return [(a, b) for a, b in merged if b - a >= min_bins], q32, q64, margin


def oracle_scores(events, counts, e_max, refs, cover, steps):
    """events / refs: per recording lists of (a, b); counts: the true event counts -> (record, per-recording records) as int lists"""
    recs, off = [], 0
    for r, s_r in enumerate(steps):
        clamp = lambda iv: (min(max(iv[0], 0), s_r), min(max(iv[1], min(max(iv[0], 0), s_r)), s_r))     # noqa: E731
        hyp = [clamp(e) for e in events[r][:min(counts[r], e_max)]]
        ref = [clamp(e) for e in refs[r]]
        over = lambda x, y: max(x[0], y[0]) < min(x[1], y[1])     # noqa: E731
        tp = fp = fn = tn = cov = 0
        for j in range(s_r):
            if cover[off + j] <= 0:
                continue
            pos, pred = any(a <= j < b for a, b in ref), any(a <= j < b for a, b in hyp)
            cov += 1
            tp += pos and pred
            fp += (not pos) and pred
            fn += pos and not pred
            tn += (not pos) and not pred
        recs.append([len(ref), len(hyp), sum(any(over(x, y) for y in hyp) for x in ref), sum(any(over(x, y) for y in ref) for x in hyp),
                     cov, tp, fp, fn, tn, int(counts[r] > e_max)])
        off += s_r
    return [sum(w) for w in zip(*recs)], recs


# ---- 1. the builders (no device) -------------------------------------------------------------------------------------------------------
def check_builders():
    from eeg_gnn_ssl_amd import annotation_bins, clip_labels_detection, clip_table_scan
    samples = [s * W + 7 for s in SMALL]                                  # (samples behind the last whole step are ignored)
    starts = lambda table, off: [[int(v) // W for v in table[off[r]:off[r + 1], 1]] for r in range(len(off) - 1)]     # noqa: E731
    table, off = clip_table_scan(samples, T, 2, W)
    assert starts(table, off) == [[], [0], [0, 1], [0, 2, 4, 5], [0, 2, 4, 6, 8, 10]] and off.tolist() == [0, 0, 1, 3, 7, 13]
    assert table.dtype == np.int64 and off.dtype == np.int64 and table.shape == (13, 4)
    assert (table[:, 2] == T * W).all() and (table[:, 3] == 0).all() and table[:, 0].tolist() == [1, 2, 2] + [3] * 4 + [4] * 6
    table, off = clip_table_scan(samples, T, 1, W)
    assert starts(table, off) == [[], [0], [0, 1], list(range(6)), list(range(11))]
    table, off = clip_table_scan(samples, T, T, W)
    assert starts(table, off) == [[], [0], [0, 1], [0, 4, 5], [0, 4, 8, 10]]
    table, off = clip_table_scan(samples, T, 2, W, cover_tail=False)
    assert starts(table, off) == [[], [0], [0], [0, 2, 4], [0, 2, 4, 6, 8, 10]]
    table, off = clip_table_scan([3 * W], T, 2, W)
    assert table.shape == (0, 4) and off.tolist() == [0, 0]
    for stride in (0, T + 1, -1):
        with pytest.raises(ValueError, match=rf"clip_table_scan: stride_steps={stride} outside 1\.\.x_steps={T}"):
            clip_table_scan(samples, T, stride, W)
    with pytest.raises(ValueError, match=r"clip_table_scan: x_steps=0"):
        clip_table_scan(samples, 0, 1, W)
    with pytest.raises(ValueError, match=r"clip_table_scan: rec_samples must name at least one recording"):
        clip_table_scan([], T, 1, W)
    # the clip label: a literal transcription of computeSliceMatrix's loop on integer sample indices
    table, off = clip_table_scan([14 * W, 9 * W], T, 2, W)
    times = [[(4.0, 5.0), (11.999, 12.5)], [(8.0, 8.5)]]
    want = []
    for rec, start_window, x_samples, _ in table.tolist():
        end_window = start_window + x_samples
        is_seizure = 0
        for t in times[rec]:
            start_t = int(t[0] * 200)
            end_t = int(t[1] * 200)
            if not ((end_window < start_t) or (start_window > end_t)):
                is_seizure = 1
                break
        want.append(is_seizure)
    got = clip_labels_detection(table, times)
    assert got.dtype == np.float32 and got.tolist() == want and 0 < sum(want) < len(want)
    # end_window == start_t: the clip [0, 800) against a seizure from 4.0 s = sample 800; start_window == end_t: the clip starting at
    # sample 1000 = 5.0 s: both count
    assert got[0] == 1.0 and int(table[0, 1]) + T * W == int(4.0 * 200)
    one = np.array([[0, 1000, 800, 0], [0, 1001, 800, 0], [0, 0, 799, 0]], dtype=np.int64)
    assert clip_labels_detection(one, [[(4.0, 5.0)]]).tolist() == [1.0, 0.0, 0.0]
    assert clip_labels_detection(torch.from_numpy(one), [[]]).tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match=r"clip_labels_detection: clip 0 names recording rec=0, seizure_times has 0"):
        clip_labels_detection(one, [])
    # annotations as bins: floor / ceil, clipping, dropping, merging (overlapping and touching), sorting, an empty result
    ref, cnt = annotation_bins([[(6.2, 7.0), (1.5, 2.2), (2.9, 3.0), (3.0, 4.5), (13.5, 99.0), (-3.0, -1.0)], [], [(20.0, 30.0)]],
                               [14 * W + 5, 9 * W, 5 * W], W)
    assert ref.dtype == np.int32 and cnt.dtype == np.int32 and cnt.tolist() == [3, 0, 0] and ref.shape == (3, 3, 2)
    assert ref[0].tolist() == [[1, 5], [6, 7], [13, 14]] and not ref[1:].any()
    ref, cnt = annotation_bins([[], []], [W, W], W)
    assert ref.shape == (2, 1, 2) and cnt.tolist() == [0, 0] and not ref.any()
    ref, cnt = annotation_bins([[(0.5, 1.0)]], [4 * 100], 100)             # (bins of half a second)
    assert ref[0].tolist() == [[1, 2]] and cnt.tolist() == [1]
    with pytest.raises(ValueError, match=r"annotation_bins: seizure_times names 1 recordings, rec_samples 2"):
        annotation_bins([[]], [W, W], W)


# ---- 2. the timeline -------------------------------------------------------------------------------------------------------------------
def _scan_case(ops, device, stride=S_STRIDE, cover_tail=True, seed=3):
    from eeg_gnn_ssl_amd import clip_table_scan
    steps = rec_steps(ops)
    table, off = clip_table_scan([s * W for s in steps], T, stride, W, cover_tail)
    g = torch.Generator().manual_seed(seed)
    probs = torch.randint(0, 257, (len(table),), generator=g).float() / 256.0
    return steps, table, off, probs


def check_timeline(device):
    """S = [3, 4, 5, 9, 14, CHUNK + 3], T = 4: stride 2 with the tail row, stride 3 without it (uncovered bins INSIDE covered
    recordings), stride 1 (cover up to 4: powers of two and 3); mean and max; outputs poisoned with NaN / -1 come back fully defined"""
    from eeg_gnn_ssl_amd import ops
    exact_bins = 0
    for stride, tail in ((2, True), (3, False), (1, True)):
        steps, table, off, probs = _scan_case(ops, device, stride, tail)
        d = lambda a: torch.as_tensor(a).to(device)     # noqa: E731
        for agg in ("mean", "max"):
            buf = ops.scan_buffers(steps, 4, device)
            buf.timeline.fill_(float("nan"))
            buf.cover.fill_(-1)
            ops.scan_timeline(d(probs), d(table), d(off), buf.bin_off, buf.timeline, buf.cover, x_steps=T, window=W, agg=agg)
            want, cover, exact = oracle_timeline(probs.numpy(), table, off, steps, T, W, agg)
            got, got_cover = buf.timeline.cpu().numpy(), buf.cover.cpu().numpy()
            assert np.array_equal(got_cover, cover) and not np.isnan(got).any()
            assert (got[cover == 0] == 0).all() and (cover[:3] == 0).all()                 # (recording 0 is shorter than T: no clip)
            if not tail:
                assert (cover[sum(steps[:3]):] == 0).any()
            if agg == "max":
                assert np.array_equal(got, want)
                continue
            want32 = exact.astype(np.float32)
            assert (np.abs(got.astype(np.float64) - want32) <= np.spacing(want32)).all()
            pow2 = (cover > 0) & ((cover & (cover - 1)) == 0)
            assert np.array_equal(got[pow2], want32[pow2]) and np.array_equal(got, want)
            exact_bins += int(pow2.sum())
            assert stride != 1 or {1, 2, 3, 4} <= set(cover.tolist())
    assert exact_bins > 3 * 1000


# ---- 3. events -------------------------------------------------------------------------------------------------------------------------
def run_events(device, timelines, covers=None, e_max=8, guard=0, **kw):
    """`ops.scan_events` on hand-made timelines (one float array per recording; covers: 0/1 arrays, default all covered) against
    the oracle: events and counts equal, smoothed within its bound, the margin condition asserted.  -> (events per recording, buffers)"""
    from eeg_gnn_ssl_amd import ops
    kw = dict(dict(smooth_bins=1, th_on=TH_ON, th_off=TH_OFF, merge_gap=0, min_bins=1), **kw)
    timelines = [np.asarray(t, dtype=np.float32) for t in timelines]
    covers = [np.ones(len(t), dtype=np.int32) if c is None else np.asarray(c, dtype=np.int32) for t, c in
              zip(timelines, covers or [None] * len(timelines))]
    steps = [len(t) for t in timelines]
    buf = ops.scan_buffers(steps, e_max, device)
    buf.timeline.copy_(torch.from_numpy(np.concatenate(timelines)))
    buf.cover.copy_(torch.from_numpy(np.concatenate(covers)))
    buf.smoothed.fill_(float("nan"))
    buf.event_count.fill_(-1)
    sentinel = -77
    store = torch.full((len(steps) * e_max * 2 + 2 * guard,), sentinel, dtype=torch.int32, device=device)
    buf.events = store[guard:store.numel() - guard].view(len(steps), e_max, 2)
    ops.scan_events(buf.timeline, buf.cover, buf.bin_off, buf.smoothed, buf.events, buf.event_count, **kw)
    got_ev, got_n, got_q = buf.events.cpu().numpy(), buf.event_count.cpu().tolist(), buf.smoothed.cpu().numpy()
    if guard:
        assert bool((store[:guard] == sentinel).all()) and bool((store[-guard:] == sentinel).all())
    out, off = [], 0
    for r, (tl, cv) in enumerate(zip(timelines, covers)):
        want, q32, q64, margin = oracle_events(tl, cv, kw["smooth_bins"], kw["th_on"], kw["th_off"], kw["merge_gap"], kw["min_bins"])
        assert margin >= MARGIN, (r, margin)
        assert got_n[r] == len(want), (r, got_n[r], want)
        kept = want[:e_max]
        assert got_ev[r, :len(kept)].tolist() == [list(e) for e in kept], (r, got_ev[r].tolist(), want)
        assert not got_ev[r, len(kept):].any()
        q = got_q[off:off + len(tl)]
        assert not np.isnan(q).any() and (np.abs(q.astype(np.float64) - q64) <= (kw["smooth_bins"] + 2) * 2.0 ** -24).all()
        assert (q[cv == 0] == 0).all()
        out.append(want)
        off += len(tl)
    return out, buf


def _long(ops, on_ranges, base=0.1):
    tl = np.full(ops.SCAN_CHUNK_BINS + 3, base, dtype=np.float32)
    for a, b in on_ranges:
        tl[a:b] = 0.9
    return tl


def check_events_rules(device):
    """hand-written timelines, one rule each (on 0.9, band 0.5, off 0.1 against th_on 0.7 / th_off 0.3)"""
    from eeg_gnn_ssl_amd import ops
    c = ops.SCAN_CHUNK_BINS
    on, mid, off = 0.9, 0.5, 0.1
    # hysteresis holds through the band in both directions; the second event is open at the recording's end
    ev, _ = run_events(device, [[off, on, mid, mid, off, mid, on, mid]])
    assert ev == [[(1, 4), (6, 8)]]
    # an uncovered bin breaks an event, and hysteresis does not carry across it
    ev, _ = run_events(device, [[on, on, on, mid, on]], [[1, 1, 0, 1, 1]])
    assert ev == [[(0, 2), (4, 5)]]
    # merging as a chain of three: gaps 1 and 2 merge under merge_gap = 2, the gap of 3 does not; merge_gap = 0 merges nothing
    chain = [off, on, on, off, on, on, off, off, on, off, off, off, on]
    ev, _ = run_events(device, [chain], merge_gap=2)
    assert ev == [[(1, 9), (12, 13)]]
    ev, _ = run_events(device, [chain])
    assert ev == [[(1, 3), (4, 6), (8, 9), (12, 13)]]
    # min_bins counts the MERGED event: two runs of one bin make an event of three; an isolated run of two is dropped
    ev, _ = run_events(device, [[off, on, off, on, off, off, off, on, on, off]], merge_gap=1, min_bins=3)
    assert ev == [[(1, 4)]]
    ev, _ = run_events(device, [[off, on, off, on, off, off, off, on, on, off]], min_bins=2)
    assert ev == [[(7, 9)]]
    # the chunk boundary: an event across it; a run that ends exactly on it and one that starts exactly on it (two recordings); a
    # merge across it; a band bin right behind it that holds the carried state; short recordings and an empty timeline beside them
    ev, _ = run_events(device, [_long(ops, [(c - 2, c + 2)]), _long(ops, [(c - 3, c)]), _long(ops, [(c, c + 2)]), [on, on, off]])
    assert ev == [[(c - 2, c + 2)], [(c - 3, c)], [(c, c + 2)], [(0, 2)]]
    ev, _ = run_events(device, [_long(ops, [(c - 2, c - 1), (c + 1, c + 3)])], merge_gap=2, min_bins=5)
    assert ev == [[(c - 2, c + 3)]]
    held = _long(ops, [(c - 1, c)])
    held[c] = mid
    ev, _ = run_events(device, [held, _long(ops, [(0, c + 3)])])
    assert ev == [[(c - 1, c + 1)], [(0, c + 3)]]
    # smooth_bins = 3: the window is cut at both ends of a recording and skips an uncovered bin (which itself stays 0 and off)
    tl, cv = [on, off, off, on, on, on, off, on], [1, 1, 1, 1, 0, 1, 1, 1]
    ev, buf = run_events(device, [tl, [on, on]], [cv, None], smooth_bins=3, th_on=0.45, th_off=0.45)
    q = buf.smoothed.cpu().numpy()
    f = np.float32
    assert q[0] == f(f(f(on) + f(off)) / f(2)) and q[3] == f(f(f(off) + f(on)) / f(2)) and q[4] == 0 and q[7] == f(f(f(off) + f(on)) / f(2))
    assert ev == [[(0, 1), (3, 4), (5, 8)], [(0, 2)]]
    assert bool((run_events(device, [tl], [cv], smooth_bins=1)[1].smoothed.cpu() == torch.tensor(tl) * torch.tensor(cv)).all())


def random_case(ops, seed):
    """the six recordings with a bimodal random timeline and about a tenth of the bins uncovered"""
    rng = np.random.default_rng(seed)
    tls, cvs = [], []
    for s_r in rec_steps(ops):
        u, v = rng.random(s_r), rng.random(s_r)
        level = np.repeat(rng.random(s_r // 5 + 1) < 0.5, 5)[:s_r]                 # stretches of high and low
        tl = np.where(u < 0.8, np.where(level, 0.75 + 0.25 * v, 0.25 * v), v).astype(np.float32)
        tls.append(tl)
        cvs.append((rng.random(s_r) > 0.1).astype(np.int32))
    return tls, cvs


RANDOM_SEEDS = (2, 12)
RANDOM_KW = dict(smooth_bins=3, th_on=0.6, th_off=0.4, merge_gap=1, min_bins=2)


def check_events_random(device):
    """seeded draws over the six recordings (the seeds are those for which the ORACLE alone meets the margin condition, found on the
    CPU; `run_events` asserts it again); E_max large enough for every event, then 5: the true counts stay, five rows are written"""
    from eeg_gnn_ssl_amd import ops
    for seed in RANDOM_SEEDS:
        tls, cvs = random_case(ops, seed)
        ev, _ = run_events(device, tls, cvs, e_max=512, guard=16, **RANDOM_KW)
        assert max(len(e) for e in ev) > 50 and len(ev[0]) <= 1
        run_events(device, tls, cvs, e_max=5, guard=16, **RANDOM_KW)
        plain, _ = run_events(device, tls, cvs, e_max=1024, th_on=0.6, th_off=0.4)
        assert sum(len(e) for e in plain) > sum(len(e) for e in ev)


def _result(device, buf, steps, refs=None):
    """a `ScanResult` from filled buffers (the scores against refs: per-recording interval lists)"""
    from eeg_gnn_ssl_amd import ScanResult, ops
    r = len(steps)
    a_max = max(1, max(len(x) for x in refs)) if refs else 1
    ref = np.zeros((r, a_max, 2), dtype=np.int32)
    for i, x in enumerate(refs or []):
        if x:
            ref[i, :len(x)] = x
    cnt = torch.tensor([len(x) for x in refs] if refs else [0] * r, dtype=torch.int32, device=device)
    ops.event_scores(buf.events, buf.event_count, torch.from_numpy(ref).to(device), cnt, buf.cover, buf.bin_off, buf.record, buf.rec_records)
    return ScanResult(torch.zeros(1, device=device), torch.zeros(r + 1, dtype=torch.int64, device=device), buf, W, 200, refs is not None)


def check_overflow(device):
    """E_max = 1 on a recording with three events: event_count == 3, one row written, the guard behind `events` untouched (checked
    in run_events), `ScanResult` raises and names the recording and its count"""
    tl = [[0.1] * 4, [0.9, 0.1, 0.9, 0.1, 0.9, 0.1]]
    ev, buf = run_events(device, tl, e_max=1, guard=32)
    assert ev[1] == [(0, 1), (2, 3), (4, 5)] and buf.event_count.tolist() == [0, 3] and buf.events.cpu().tolist() == [[[0, 0]], [[0, 1]]]
    with pytest.raises(ValueError, match=r"Scanner: recording 1 has 3 events, max_events=1 rows are kept \(1 recording\(s\) overflow\)"):
        _result(device, buf, [4, 6])
    assert buf.record.cpu().tolist()[9] == 1 and buf.rec_records.cpu()[:, 9].tolist() == [0, 1]
    ev, buf = run_events(device, tl, e_max=3)
    res = _result(device, buf, [4, 6])
    assert res.scores is None and res.events_seconds() == [(1, 0.0, 1.0), (1, 2.0, 3.0), (1, 4.0, 5.0)]
    assert res.per_recording(1)["events"].tolist() == [[0, 1], [2, 3], [4, 5]] and res.per_recording(0)["events"].shape == (0, 2)


# ---- 4. scores -------------------------------------------------------------------------------------------------------------------------
def check_scores(device):
    """hand-made events and references against the oracle's integers: a detected event over two reference events, two detected
    events inside one reference event, recordings without reference / detection / clip, uncovered bins, hostile intervals (clamped),
    an overflowing count; n_ref = 0: sensitivity NaN, nothing raises"""
    from eeg_gnn_ssl_amd import ops, scores_from_scan_record
    steps = [20, 12, 6, 3, 9]
    events = [[(2, 9), (15, 17)], [(1, 2), (4, 6)], [(0, 3)], [], []]
    counts = [2, 2, 1, 0, 0]
    refs = [[(3, 4), (7, 12)], [(0, 8)], [], [(0, 2)], []]
    e_max = 2
    buf = ops.scan_buffers(steps, e_max, device)
    cover = np.ones(sum(steps), dtype=np.int32)
    cover[5] = cover[22] = 0
    cover[38:41] = 0                                                      # (recording 3 has no clip: uncovered throughout)
    buf.cover.copy_(torch.from_numpy(cover))

    def fill(events, counts):
        ev = np.zeros((len(steps), e_max, 2), dtype=np.int32)
        for r, e in enumerate(events):
            if e:
                ev[r, :len(e[:e_max])] = e[:e_max]
        buf.events.copy_(torch.from_numpy(ev))
        buf.event_count.copy_(torch.tensor(counts, dtype=torch.int32))

    fill(events, counts)
    buf.record.fill_(-5)
    buf.rec_records.fill_(-5)
    res = _result(device, buf, steps, refs)
    want, want_recs = oracle_scores(events, counts, e_max, refs, cover, steps)
    assert res.record.tolist() == want and res.rec_records.cpu().tolist() == want_recs
    assert want[:5] == [4, 5, 3, 3, sum(steps) - 5] and want_recs[0][:4] == [2, 2, 2, 1] and want_recs[1][:4] == [1, 2, 1, 2]
    assert list(res.scores) == ["sensitivity", "false_alarms_per_24h", "n_ref", "n_hyp", "bin_precision", "bin_recall", "bin_F1"]
    tp, fp, fn = want[5:8]
    assert res.scores["sensitivity"] == 3 / 4 and res.scores["false_alarms_per_24h"] == 2 / ((sum(steps) - 5) * W / 200 / 86400.0)
    assert res.scores["bin_precision"] == tp / (tp + fp) and res.scores["bin_recall"] == tp / (tp + fn)
    assert res.scores["bin_F1"] == 2 * tp / (2 * tp + fp + fn) and (res.scores["n_ref"], res.scores["n_hyp"]) == (4, 5)
    # hostile intervals are clamped into the recording; a count above E_max scores the stored rows and flags the recording
    hostile, hostile_counts = [[(-5, 3), (18, 999)], [(7, 2), (4, 6)], [(0, 3)], [], []], [2, 7, 1, 0, -3]
    fill(hostile, hostile_counts)
    ops.event_scores(buf.events, buf.event_count, torch.tensor([[[3, 4], [7, 12]], [[0, 8], [0, 0]], [[0, 0]] * 2, [[0, 2], [0, 0]], [[0, 0]] * 2],
                                                               dtype=torch.int32, device=device),
                     torch.tensor([2, 1, 0, 1, 0], dtype=torch.int32, device=device), buf.cover, buf.bin_off, buf.record, buf.rec_records)
    want, want_recs = oracle_scores(hostile, [2, 7, 1, 0, 0], e_max, refs, cover, steps)
    assert buf.record.cpu().tolist() == want and buf.rec_records.cpu().tolist() == want_recs and want[9] == 1
    # no reference at all
    fill(events, counts)
    res = _result(device, buf, steps, [[]] * 5)
    assert res.record.tolist()[:4] == [0, 5, 0, 0] and math.isnan(res.scores["sensitivity"]) and math.isnan(res.scores["bin_recall"])
    assert res.scores["false_alarms_per_24h"] > 0 and res.scores["bin_precision"] == 0.0
    nothing = scores_from_scan_record([0] * 10, W)
    assert all(math.isnan(nothing[k]) for k in ("sensitivity", "false_alarms_per_24h", "bin_precision", "bin_recall", "bin_F1"))


# ---- 5. the pass -----------------------------------------------------------------------------------------------------------------------
PASS_LENGTHS = (2100, 1803, 600)             # 10, 9 and 3 whole steps: 4 + 4 windows (a tail row in recording 1), none in recording 2
ANNOTATIONS = ([(2.0, 6.5)], [(3.0, 4.0), (7.5, 20.0)], [(0.0, 1.0)])
POST = dict(agg="mean", smooth_bins=3, th_on=0.5, th_off=0.45, merge_gap=1, min_bins=2)


def _same_result(a, b):
    for name in ("clip_probs", "clip_off", "bin_off", "timeline", "cover", "smoothed", "events", "event_count", "record", "rec_records"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert str(a.scores) == str(b.scores)                                  # (NaN compares unequal to itself)


def _scanner_case(kind, adj3d, device, units):
    """record_pool_suite's detection step (model, parameters, raw chain, graph) over three recordings of this suite's lengths"""
    from eeg_gnn_ssl_amd import annotation_bins
    make, ds, _, supports = rp._step_case(kind, adj3d, device, units)
    recs = rp._recordings(PASS_LENGTHS, 46)
    return make, recs, ds, supports, annotation_bins(ANNOTATIONS, PASS_LENGTHS, rp.W)


def check_pass(device, adj3d, kind, units=16):
    """record_pool_suite's detection case (kind: detection = supports None, detection_shared = the distance graph), T = 4, stride 2,
    B = 3: 4 + 4 + 0 windows, the last step short, recording 2 uncovered"""
    from eeg_gnn_ssl_amd import DeviceDataset, EpochSampler, RecordingDataset
    capture = device != "cpu"
    make, recs, ds, supports, ann = _scanner_case(kind, adj3d, device, units)
    model, st = make()
    train_sampler = EpochSampler(rp.P, rp.B, 77, 0, 1, device=device)
    st.begin_epoch(0, 2, sampler=train_sampler)
    st.step_from(ds, train_sampler, supports)                                # a training step taken: Adam moments, counters, a sampler

    def state():
        return (model.training, st.step_count, st.samples_seen, st.step_dev.clone(), st.samples_seen_dev.clone(), st.fp.flat.detach().clone(),
                st.exp_avg.clone(), st.exp_avg_sq.clone(), None if st._augment_rng is None else st._augment_rng.clone(), model._dropout_rng.clone(),
                train_sampler.cursor.clone(), train_sampler._host_cursor, id(st.sampler), st.lr)

    sc = st.scanner(recs, x_steps=T, stride_steps=S_STRIDE, batch_size=3, supports=supports)
    assert len(sc.dataset) == 8 and sc.clip_off.tolist() == [0, 4, 8, 8] and sc.bin_off.tolist() == [0, 10, 19, 22]
    assert sc.sampler.steps_per_epoch == 3
    with pytest.raises(ValueError, match=r"Scanner.postprocess: no pass has run yet"):
        sc.postprocess()
    before = state()
    assert model.training and bool(st.exp_avg.abs().sum() > 0)
    res = sc.run(capture=capture, annotations=ann, **POST)
    for u, v in zip(before, state()):
        assert torch.equal(u, v) if torch.is_tensor(u) else u == v
    assert st.sampler is train_sampler
    # the probabilities: DeviceEvaluator over the same table, and over the pools pre-cut with numpy
    table = sc.dataset.clip_table.cpu().numpy()
    zeros = torch.zeros(len(table), device=device)
    ev = st.evaluator(RecordingDataset(recs, table, zeros, window=rp.W, x_steps=T, device=device), 3, supports)
    ev.run(capture=capture)
    x_pool, len_pool, _ = rp.cut_pools(recs, table, rp.W, T, 0)
    assert len_pool.tolist() == [T] * len(table)
    ev_p = st.evaluator(DeviceDataset(x_pool.to(device), zeros), 3, supports)
    ev_p.run(capture=capture)
    assert torch.equal(res.clip_probs, ev.probs) and torch.equal(res.clip_probs, ev_p.probs)
    probs = res.clip_probs.cpu().numpy()
    assert np.isfinite(probs).all() and len(set(probs.tolist())) == len(probs)
    if supports is not None:
        # ... and `predict` on the features of the pre-cut pools, at parity_suite's tolerance (what eval_pass_suite holds the evaluator
        # to against `predict`); with supports=None `predict` builds its graphs from the standardised features, the step from the raw ones
        from eeg_gnn_ssl_amd import ops
        from eeg_gnn_ssl_amd.train_step import predict
        from parity_suite import assert_close
        feats = ops.fft_features(x_pool.to(device), window=rp.W, mean=st.raw_mean, std=st.raw_std)[1]
        lens = len_pool.to(device)
        batches = [(feats[i:i + 3], zeros[i:i + 3], lens[i:i + 3], supports) for i in range(0, len(table), 3)]
        assert_close(probs, predict(model, batches, task="detection")[0], f"scan {kind}: clip probabilities against predict")
    # the post-processing against the oracle on those probabilities
    tl, cover, _ = oracle_timeline(probs, table, sc.clip_off.tolist(), sc.rec_steps, T, rp.W, "mean")
    assert np.array_equal(res.timeline.cpu().numpy(), tl) and np.array_equal(res.cover.cpu().numpy(), cover)
    assert (cover[:19] > 0).all() and not cover[19:].any()
    want_ev, got_n = [], res.event_count.tolist()
    for r in range(3):
        b0, b1 = sc.bin_off.tolist()[r:r + 2]
        e, _, _, _ = oracle_events(tl[b0:b1], cover[b0:b1], POST["smooth_bins"], POST["th_on"], POST["th_off"], POST["merge_gap"], POST["min_bins"])
        want_ev.append(e)
        if got_n[r] == len(e):                                              # (no margin is asserted on a model's outputs: print, then compare)
            assert res.per_recording(r)["events"].tolist() == [list(x) for x in e]
    print(f"scan {kind}: timeline {tl[:19].min():.4f}..{tl.max():.4f}, events {res.events_seconds()} (oracle {want_ev}), scores {dict(res.scores)}")
    assert res.record.tolist()[0] == 4 and res.record.tolist()[4] == 19 and res.scores["n_ref"] == 4
    assert res.per_recording(1)["timeline"].shape == (9,) and res.per_recording(2)["clip_probs"].shape == (0,)
    # postprocess with other arguments equals a full run with them (thresholds taken from the timeline so that there ARE events); that
    # second run has the first one's probabilities, and the first one's arguments give the first one's result again: two consecutive
    # runs are bit-equal; then the other way of issuing the steps
    lo, hi = float(np.quantile(tl[:19], 0.4)), float(np.quantile(tl[:19], 0.6))
    other = dict(agg="max", smooth_bins=1, th_on=hi, th_off=lo, merge_gap=0, min_bins=1)
    post = sc.postprocess(annotations=ann, **other)
    assert int(post.record[1]) >= 1 and not torch.equal(post.timeline, res.timeline)
    _same_result(post, sc.run(capture=capture, annotations=ann, **other))
    _same_result(res, sc.postprocess(annotations=ann, **POST))
    assert sc.postprocess(**other).scores is None
    if capture:
        _same_result(res, sc.run(capture=False, annotations=ann, **POST))


def two_rank_result(device="cpu", rank=None, world=None):
    """the scan of the two-rank check (supports None, eager): built alike in every process"""
    make, recs, _, _, ann = _scanner_case("detection", None, device, 16)
    _, st = make()
    sc = st.scanner(recs, x_steps=T, stride_steps=S_STRIDE, batch_size=3, rank=rank, world=world)
    return sc.run(capture=False, annotations=ann, **POST)


RESULT_FIELDS = ("clip_probs", "timeline", "cover", "smoothed", "events", "event_count", "record", "rec_records")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(device, adj3d, units=16):
    """every ValueError of the operators and of the scanner, by message, before any launch; the C entry points refuse the same and
    name the argument; no refused call writes"""
    from eeg_gnn_ssl_amd import _lib, ops
    from eeg_gnn_ssl_amd.train_step import TrainStep
    steps, table, off, probs = _scan_case(ops, device)
    d = lambda a: torch.as_tensor(a).to(device)     # noqa: E731
    probs, table, off = d(probs), d(table), d(off)
    buf = ops.scan_buffers(steps, 4, device)
    total = sum(steps)
    tl_args = lambda **k: dict(dict(probs=probs, clip_table=table, clip_off=off, bin_off=buf.bin_off, timeline=buf.timeline, cover=buf.cover,     # noqa: E731
                                    x_steps=T, window=W), **k)
    for change, text in (
            (dict(probs=probs.double()), r"scan_timeline: probs must be a contiguous torch.float32 tensor of shape \(\*,\)"),
            (dict(clip_table=table.int()), r"scan_timeline: clip_table must be a contiguous torch.int64 tensor"),
            (dict(clip_table=table[:-1]), r"scan_timeline: clip_off ends at \d+, the table has \d+ rows"),
            (dict(clip_table=table.t().contiguous().t()), r"scan_timeline: clip_table must be a contiguous"),
            (dict(clip_off=off[:-1]), r"scan_timeline: clip_off is not a monotone offset table from 0 to \d+"),
            (dict(clip_off=off.int()), r"scan_timeline: clip_off must be a contiguous torch.int64 tensor of shape \(7,\)"),
            (dict(timeline=buf.timeline[:-1]), r"scan_timeline: bin_off is not a monotone offset table from 0 to"),
            (dict(cover=buf.cover.long()), r"scan_timeline: cover must be a contiguous torch.int32"),
            (dict(cover=torch.zeros(total, dtype=torch.int32, device="meta")), r"scan_timeline: cover is on meta, timeline on"),
            (dict(bin_off=torch.flip(buf.bin_off, [0])), r"scan_timeline: bin_off is not a monotone offset table"),
            (dict(clip_off=torch.flip(off, [0])), r"scan_timeline: clip_off is not a monotone offset table"),
            (dict(agg="median"), r"scan_timeline: agg='median'"),
            (dict(x_steps=T + 1), r"scan_timeline: the rows of recording 1 are not all x_steps\*window = 1000 samples long"),
            (dict(clip_table=torch.flip(table, [0])), r"scan_timeline: rows 0\.\.1 of the table belong to recording 1 by clip_off and name another"),
    ):
        with pytest.raises(ValueError, match=text):
            ops.scan_timeline(**tl_args(**change))
    swapped = table.clone()
    swapped[[3, 4]] = swapped[[4, 3]]                                      # recording 3's rows no longer ascend
    with pytest.raises(ValueError, match=r"scan_timeline: the rows of recording 3 do not start at whole, ascending steps"):
        ops.scan_timeline(**tl_args(clip_table=swapped))
    odd = table.clone()
    odd[1, 1] += 1
    with pytest.raises(ValueError, match=r"scan_timeline: the rows of recording 2 do not start at whole, ascending steps"):
        ops.scan_timeline(**tl_args(clip_table=odd))
    ev_args = lambda **k: dict(dict(timeline=buf.timeline, cover=buf.cover, bin_off=buf.bin_off, smoothed=buf.smoothed, events=buf.events,     # noqa: E731
                                    event_count=buf.event_count), **k)
    for change, text in (
            (dict(smooth_bins=2), r"scan_events: smooth_bins=2 must be odd"),
            (dict(smooth_bins=0), r"scan_events: smooth_bins=0 must be odd"),
            (dict(smooth_bins=ops.SCAN_MAX_SMOOTH_BINS + 2), r"scan_events: smooth_bins=131 must be odd, 1\.\.129"),
            (dict(th_on=0.4, th_off=0.5), r"scan_events: th_off=0.5 above th_on=0.4"),
            (dict(th_on=float("nan")), r"scan_events: a threshold is NaN"),
            (dict(th_off=float("nan")), r"scan_events: a threshold is NaN"),
            (dict(merge_gap=-1), r"scan_events: merge_gap=-1"),
            (dict(min_bins=0), r"scan_events: merge_gap=0 \(>= 0\), min_bins=0"),
            (dict(events=buf.events[:, :0]), r"scan_events: events must be \(R, E_max, 2\) int32 with E_max >= 1"),
            (dict(events=buf.events.long()), r"scan_events: events must be a contiguous torch.int32"),
            (dict(events=buf.events[:, ::2]), r"scan_events: events must be a contiguous"),
            (dict(event_count=buf.event_count[:-1]), r"scan_events: event_count must be a contiguous torch.int32 tensor of shape \(6,\)"),
            (dict(smoothed=buf.smoothed.double()), r"scan_events: smoothed must be a contiguous torch.float32"),
            (dict(cover=buf.cover.float()), r"scan_events: cover must be a contiguous torch.int32"),
            (dict(bin_off=buf.bin_off.int()), r"scan_events: bin_off must be a contiguous torch.int64"),
            (dict(bin_off=buf.bin_off - 1), r"scan_events: bin_off is not a monotone offset table from 0"),
            (dict(timeline=torch.zeros(total, device="meta")), r"scan_events: cover is on .*, timeline on meta"),
    ):
        with pytest.raises(ValueError, match=text):
            ops.scan_events(**ev_args(**change))
    ref, cnt = torch.zeros(len(steps), 2, 2, dtype=torch.int32, device=device), torch.zeros(len(steps), dtype=torch.int32, device=device)
    sc_args = lambda **k: dict(dict(events=buf.events, event_count=buf.event_count, ref=ref, ref_count=cnt, cover=buf.cover, bin_off=buf.bin_off,     # noqa: E731
                                    record=buf.record, rec_records=buf.rec_records), **k)
    for change, text in (
            (dict(ref=ref[:-1]), r"event_scores: ref must be a contiguous torch.int32 tensor of shape \(6, \*, 2\)"),
            (dict(ref=ref[:, :0]), r"event_scores: ref must be a contiguous torch.int32"),
            (dict(ref_count=cnt.long()), r"event_scores: ref_count must be a contiguous torch.int32"),
            (dict(record=buf.record[:-1]), r"event_scores: record must be a contiguous torch.int64 tensor of shape \(10,\)"),
            (dict(rec_records=buf.rec_records.t()), r"event_scores: rec_records must be a contiguous torch.int64 tensor of shape \(6, 10\)"),
            (dict(bin_off=torch.flip(buf.bin_off, [0])), r"event_scores: bin_off is not a monotone offset table"),
            (dict(cover=buf.cover[:-2]), r"event_scores: bin_off is not a monotone offset table from 0 to"),
    ):
        with pytest.raises(ValueError, match=text):
            ops.event_scores(**sc_args(**change))
    for bad, text in (((steps, 0), r"scan_buffers: max_events=0: E_max < 1"), (([], 4), r"scan_buffers: rec_steps names 0 recordings"),
                      (([0, 0], 4), r"scan_buffers: the recordings hold 0 whole steps"), (([3, -1], 4), r"scan_buffers: rec_steps names 2 recordings")):
        with pytest.raises(ValueError, match=text):
            ops.scan_buffers(*bad, device)
    for t in (buf.timeline, buf.smoothed, buf.cover, buf.events, buf.event_count, buf.record, buf.rec_records):
        assert not bool(t.any())                                           # no refused call wrote anything
    # the scanner
    recs = rp._recordings(rp.STEP_LENGTHS, 44)
    make, _, _, supports = rp._step_case("detection", adj3d, device, units)
    model, st = make()
    with pytest.raises(ValueError, match=r"Scanner: the step has raw_window=None"):
        TrainStep(make()[0], task="detection").scanner(recs, x_steps=T, stride_steps=2)
    for kind, text in (("classification", r"Scanner: task='classification': .* TrainStep.evaluator$"),
                       ("ssl", r"Scanner: task='ssl': .* TrainStep.evaluator / TrainStep.ssl_evaluator$")):
        with pytest.raises(ValueError, match=text):
            rp._step_case(kind, adj3d, device, units)[0]()[1].scanner(recs, x_steps=T, stride_steps=2)
    four = rp._step_case("classification", adj3d, device, units)[0]()[0]
    with pytest.raises(ValueError, match=r"Scanner: the model's head has 4 outputs; a detector has one"):
        TrainStep(four, task="detection", raw_window=rp.W).scanner(recs, x_steps=T, stride_steps=2)
    for kw, text in ((dict(x_steps=T, stride_steps=T + 1), r"clip_table_scan: stride_steps=5 outside 1\.\.x_steps=4"),
                     (dict(x_steps=26, stride_steps=1), r"Scanner: no recording holds x_steps=26 whole steps of 200 samples \(the longest has 25\)"),
                     (dict(x_steps=T, stride_steps=2, max_events=0), r"Scanner: max_events=0"),
                     (dict(x_steps=T, stride_steps=2, batch_size=0), r"Scanner: batch_size=0")):
        with pytest.raises(ValueError, match=text):
            st.scanner(recs, **kw)
    sc = st.scanner(recs, x_steps=T, stride_steps=2, batch_size=8)
    for kw, text in ((dict(agg="median"), r"Scanner: agg='median'"), (dict(smooth_bins=4), r"Scanner: smooth_bins=4 must be odd"),
                     (dict(th_on=0.2, th_off=0.3), r"scan_events: th_off=0.3 above th_on=0.2"), (dict(th_on=float("nan")), r"a threshold is NaN"),
                     (dict(min_bins=0), r"Scanner: merge_gap=0 \(>= 0\), min_bins=0"),
                     (dict(annotations=(np.zeros((2, 1, 2), dtype=np.int32), np.zeros(2, dtype=np.int32))), r"Scanner: annotations must be \(ref \(R, A_max, 2\)")):
        with pytest.raises(ValueError, match=text):
            sc.run(capture=False, **kw)
    assert not sc._passed and not bool(sc.probs.any())                     # refused before the pass
    # a scanner over the (signals, rec_table, num_channels) of a data set
    ds = rp._step_case("detection", adj3d, device, units)[1]
    again = st.scanner((ds.signals, ds.rec_table, ds.N), x_steps=T, stride_steps=2, batch_size=8)
    assert again.dataset.signals.data_ptr() == ds.signals.data_ptr() and torch.equal(again.dataset.clip_table, sc.dataset.clip_table)
    # the C entry points
    lib = _lib.get_lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())     # noqa: E731
    r = len(steps)

    def refused(rc, text):
        assert rc != 0 and text in lib.last_error(), (rc, lib.last_error())

    def timeline(probs_=p(probs), n=len(probs), r_=r, total_=total, t=T, w=W, agg=0, out=p(buf.timeline), cover=p(buf.cover)):
        return lib.query("eeg_dcrnn_scan_timeline", probs_, n, p(table), p(off), p(buf.bin_off), r_, total_, t, w, agg, out, cover, None)

    refused(timeline(probs_=None), "null probs / clip_table / clip_off / bin_off")
    refused(timeline(out=None), "null timeline / cover")
    refused(timeline(n=0), "P=0 clips")
    refused(timeline(n=ops.EVAL_MAX_CLIPS + 1), f"P={ops.EVAL_MAX_CLIPS + 1}")
    refused(timeline(r_=0), "R=0 recordings")
    refused(timeline(total_=0), "total_bins=0")
    refused(timeline(total_=2 ** 31), "total_bins=2147483648")
    refused(timeline(t=0), "x_steps=0")
    refused(timeline(w=0), "window=0")
    refused(timeline(agg=2), "agg=2")
    refused(timeline(cover=ctypes.c_void_p(buf.cover.data_ptr() + 2)), "aligned to their element size")

    def events(sm=1, on=0.5, off_=0.5, gap=0, mn=1, e=4, out=p(buf.events), r_=r):
        return lib.query("eeg_dcrnn_scan_events", p(buf.timeline), p(buf.cover), p(buf.bin_off), r_, total, sm, on, off_, gap, mn, e, p(buf.smoothed),
                         out, p(buf.event_count), None)

    refused(events(out=None), "null smoothed / events / event_count")
    refused(events(sm=2), "smooth_bins=2 unsupported")
    refused(events(sm=131), "smooth_bins=131 unsupported")
    refused(events(on=float("nan")), "a threshold is NaN")
    refused(events(on=0.25, off_=0.5), "th_off=0.5 above th_on=0.25")
    refused(events(gap=-1), "merge_gap=-1")
    refused(events(mn=0), "min_bins=0")
    refused(events(e=0), "E_max=0")
    refused(events(r_=ops.SCAN_MAX_RECORDINGS + 1), f"R={ops.SCAN_MAX_RECORDINGS + 1}")

    def scores(e=4, a=2, rec=p(buf.record), ref_=p(ref)):
        return lib.query("eeg_dcrnn_event_scores", p(buf.events), p(buf.event_count), e, ref_, p(cnt), a, p(buf.cover), p(buf.bin_off), r, total, rec,
                         p(buf.rec_records), None)

    refused(scores(ref_=None), "null events / event_count / ref / ref_count")
    refused(scores(rec=None), "null cover / bin_off / record / rec_records")
    refused(scores(e=0), "E_max=0")
    refused(scores(a=0), "A_max=0")
    refused(scores(rec=ctypes.c_void_p(buf.record.data_ptr() + 4)), "aligned to their element size")
    for t in (buf.timeline, buf.smoothed, buf.cover, buf.events, buf.event_count, buf.record, buf.rec_records):
        assert not bool(t.any())


def check_hostile_tables():
    """emulator only: the C entry points on tables no host check has seen -- starts far outside the recordings, clip and bin offsets
    that decrease, go negative or run past the buffers, counts beyond E_max / A_max, intervals outside the recording -- with guard
    regions around every output: each call either refuses cleanly or returns 0 with every guard intact and every output defined"""
    from eeg_gnn_ssl_amd import _lib, ops
    lib = _lib.get_lib()
    assert not lib.is_device_build
    p = lambda x: ctypes.c_void_p(x.data_ptr())     # noqa: E731
    steps, table, off, probs = _scan_case(ops, "cpu")
    r, total, n, guard, e_max, a_max = len(steps), sum(steps), len(probs), 64, 3, 2
    bin_off = torch.tensor(np.concatenate([[0], np.cumsum(steps)]), dtype=torch.int64)
    table, off = torch.from_numpy(table), torch.from_numpy(off)
    big = 2 ** 62

    def guarded(count, dtype, fill):
        store = torch.full((count + 2 * guard,), fill, dtype=dtype)
        return store, store[guard:guard + count]

    tables = []
    for k in range(6):
        tb, co, bo = table.clone(), off.clone(), bin_off.clone()
        if k == 0:
            tb[:, 1] = torch.tensor([big, -big, -1, 10 ** 9] * n)[:n]
        elif k == 1:
            co[:] = torch.tensor([0, n + 50, -7, big, 3, -big, n])
        elif k == 2:
            bo[:] = torch.tensor([0, total + 99, -5, big, 2, -big, total])
        elif k == 3:
            co, bo = torch.flip(co, [0]), torch.flip(bo, [0])
        elif k == 4:
            tb[:, 1] = torch.flip(tb[:, 1], [0])
            tb[:, 0] = 10 ** 6
        else:
            bo[:] = total                                                  # every recording empty
        tables.append((tb, co, bo))
    events_in = torch.tensor([[[-9, 4], [2, 2 ** 31 - 1], [7, 1]]] * r, dtype=torch.int32)
    refs_in = events_in[:, :a_max].contiguous()
    for tb, co, bo in tables:
        for agg in (0, 1):
            s_tl, tl = guarded(total, torch.float32, float("nan"))
            s_cv, cv = guarded(total, torch.int32, -1)
            rc = lib.query("eeg_dcrnn_scan_timeline", p(probs), n, p(tb), p(co), p(bo), r, total, T, W, agg, p(tl), p(cv), None)
            assert rc == 0, lib.last_error()
            assert bool(torch.isnan(s_tl[:guard]).all()) and bool(torch.isnan(s_tl[-guard:]).all()) and not bool(torch.isnan(tl).any())
            assert bool((s_cv[:guard] == -1).all()) and bool((s_cv[-guard:] == -1).all()) and bool(((cv >= 0) & (cv <= n)).all())
            assert bool((tl[cv == 0] == 0).all()) and bool(((tl >= 0) & (tl <= 1)).all())
        s_sm, sm = guarded(total, torch.float32, float("nan"))
        s_ev, ev = guarded(r * e_max * 2, torch.int32, -77)
        s_ec, ec = guarded(r, torch.int32, -77)
        tl.copy_(torch.rand(total, generator=torch.Generator().manual_seed(1)))
        rc = lib.query("eeg_dcrnn_scan_events", p(tl), p(cv), p(bo), r, total, 3, 0.6, 0.4, 1, 1, e_max, p(sm), p(ev), p(ec), None)
        assert rc == 0, lib.last_error()
        for store in (s_ev, s_ec):
            assert bool((store[:guard] == -77).all()) and bool((store[-guard:] == -77).all())
        assert bool(torch.isnan(s_sm[:guard]).all()) and bool(torch.isnan(s_sm[-guard:]).all())
        assert bool((ev != -77).all()) and bool((ec >= 0).all())
        s_rec, rec = guarded(ops.SCAN_RECORD_WORDS, torch.int64, -77)
        s_rr, rr = guarded(r * ops.SCAN_RECORD_WORDS, torch.int64, -77)
        counts = torch.tensor([-4, 0, 99, 3, 2 ** 31 - 1, 1], dtype=torch.int32)
        rc = lib.query("eeg_dcrnn_event_scores", p(events_in), p(counts), e_max, p(refs_in), p(counts), a_max, p(cv), p(bo),
                       r, total, p(rec), p(rr), None)
        assert rc == 0, lib.last_error()
        for store in (s_rec, s_rr):
            assert bool((store[:guard] == -77).all()) and bool((store[-guard:] == -77).all())
        assert bool((rec >= 0).all()) and bool((rr >= 0).all()) and rec.tolist() == rr.view(r, -1).sum(0).tolist()
        assert int(rec[0]) <= r * a_max and int(rec[1]) <= r * e_max and int(rec[4]) <= total


# ---- 7. operator registration ------------------------------------------------------------------------------------------------------------
def check_opcheck(device):
    """`torch.library.opcheck` (schema incl. the declared mutations, autograd registration, fake implementation) on the three operators"""
    from eeg_gnn_ssl_amd import clip_table_scan, ops
    E = torch.ops.eeg_dcrnn
    steps = SMALL
    table, off = clip_table_scan([s * W for s in steps], T, S_STRIDE, W)
    d = lambda a: torch.as_tensor(a).to(device)     # noqa: E731
    g = torch.Generator().manual_seed(4)
    buf = ops.scan_buffers(steps, 3, device)
    filled = ops.scan_buffers(steps, 3, device)
    filled.timeline.copy_(torch.rand(sum(steps), generator=g))
    filled.cover.fill_(1)
    filled.events.copy_(torch.tensor([[[0, 1], [0, 0], [0, 0]]] * len(steps), dtype=torch.int32))
    filled.event_count.fill_(1)
    ref, cnt = d(torch.tensor([[[0, 2]]] * len(steps), dtype=torch.int32)), d(torch.ones(len(steps), dtype=torch.int32))
    samples = [
        (E.scan_timeline.default, (d(torch.rand(len(table), generator=g)), d(table), d(off), buf.bin_off, T, W, 0, buf.timeline, buf.cover)),
        (E.scan_timeline.default, (d(torch.rand(len(table), generator=g)), d(table), d(off), buf.bin_off, T, W, 1, buf.timeline, buf.cover)),
        (E.scan_events.default, (filled.timeline, filled.cover, filled.bin_off, 3, 0.6, 0.4, 1, 1, buf.smoothed, buf.events, buf.event_count)),
        (E.event_scores.default, (filled.events, filled.event_count, ref, cnt, filled.cover, filled.bin_off, buf.record, buf.rec_records)),
    ]
    for op, args in samples:
        res = torch.library.opcheck(op, args, test_utils=["test_schema", "test_autograd_registration", "test_faketensor"], raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (str(op), res)
