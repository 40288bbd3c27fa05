"""GPU: the calibration kernels (csrc/calib.hip) against ``calib_ref`` within its derived bounds -- ``ss_calib_moments`` at its
class-count, row-count and grid-stride edges, the enqueue-only fit, ``ss_calib_bins`` on rows whose confidence sits at a bin centre,
``ss_softmax_topk_t`` bit for bit against ``ss_softmax_topk`` at u = 1 and within the bound elsewhere -- the launch lists of the
serving calls with and without a temperature, and ``harness.fit_calibrated`` end to end."""
import math
import types

import numpy as np
import pytest
import torch

import calib_ref as CR
import launch_trace as LT
from gpu_support import L, WORDS, cuda, ss, sync, write_clips  # noqa: F401

pytestmark = pytest.mark.gpu


def make_logits(seed, N, C, scale=3.0, p_right=0.7):
    rng = np.random.default_rng(seed)
    z = (scale * rng.normal(size=(N, C))).astype(np.float32)
    y = np.where(rng.random(N) < p_right, z.argmax(1), rng.integers(0, C, N)).astype(np.int64)
    return z, y


def run_moments(L, z, y, u):
    """One ss_calib_moments launch at inverse temperature u, its slots summed on the host -> (sum nll, sum g, flag, partials)."""
    from silent_speech_amd import calibrate as Cal

    N, C = z.shape
    n_part = Cal.n_partials_for(N)
    z_d, y_d = cuda(torch.from_numpy(z)), cuda(torch.from_numpy(y))
    state = Cal.new_state("cuda")
    state[0] = u
    partials = torch.full((2 * n_part,), float("nan"), dtype=torch.float64, device="cuda")  # every slot must be written
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("ss_calib_moments", z_d.data_ptr(), y_d.data_ptr(), N, C, state.data_ptr(), partials.data_ptr(), n_part, err.data_ptr(),
           L.stream())
    sync()
    p = partials.cpu().numpy()
    return float(p[0::2].sum()), float(p[1::2].sum()), int(err), p


def check_moments(L, z, y, u, what, y_ref=None, rows=None):
    nll, g, flag, p = run_moments(L, z, y, u)
    zr, yr = (z, y) if rows is None else (z[rows], y_ref[rows])
    want_nll, want_g = CR.moments(zr, yr, u)
    b = CR.bounds(zr, yr, u)
    print(f"moments {what} u={u}: nll err / bound {abs(nll - want_nll) / b['nll_sum']:.4f}, g err / bound "
          f"{abs(g - want_g) / b['g_sum']:.4f}")
    assert np.isfinite(p).all(), what
    assert abs(nll - want_nll) <= b["nll_sum"], (what, nll, want_nll, b["nll_sum"])
    assert abs(g - want_g) <= b["g_sum"], (what, g, want_g, b["g_sum"])
    return flag, p


# ---------------------------------------------------------------------------------------------------------- ss_calib_moments
@pytest.mark.parametrize("C", [2, 3, 63, 64, 65, 130])
def test_moments_against_the_reference(L, C):
    for N in (1, 3, 4, 5):
        z, y = make_logits(100 * C + N, N, C)
        for u in (0.3, 1.0, 2.5):
            flag, _ = check_moments(L, z, y, u, f"C={C} N={N}")
            assert flag == 0


def test_moments_at_the_grid_stride_cap(L):
    from silent_speech_amd import calibrate as Cal

    G = Cal.MAX_PARTIALS
    for N in (4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 3):
        z, y = make_logits(N, N, 3)
        flag, p = check_moments(L, z, y, 1.7, f"N={N}")
        assert flag == 0 and len(p) == 2 * G
        _, _, _, p2 = run_moments(L, z, y, 1.7)
        assert p.tobytes() == p2.tobytes(), "two runs on the same input must be bit-equal"


def test_moments_skips_rows_with_a_bad_label_and_raises_the_flag(L):
    from silent_speech_amd import calibrate as Cal

    N = 4 * Cal.MAX_PARTIALS + 9  # more than one pass of the grid: the last row belongs to a second sweep
    z, y = make_logits(7, N, 5)
    bad = y.copy()
    bad[0], bad[N // 2], bad[N - 1] = -1, 5, 2 ** 33 + 1   # (the last one is a valid index once truncated to 32 bits)
    rows = np.setdiff1d(np.arange(N), [0, N // 2, N - 1])
    flag, p = check_moments(L, z, bad, 0.8, "bad labels", y_ref=y, rows=rows)
    assert flag == 1
    assert run_moments(L, z, bad, 0.8)[3].tobytes() == p.tobytes()
    assert run_moments(L, z, y, 0.8)[2] == 0
    lib = L.load()
    assert lib.ss_calib_moments(8, 8, 4, 1, 8, 8, 1, 8, None) == -1  # one class: refused before any launch


# -------------------------------------------------------------------------------------------------------------------- the fit
def fit_on_device(z, y):
    from silent_speech_amd import calibrate as Cal

    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = Cal.fit_temperature(cuda(torch.from_numpy(z)), cuda(torch.from_numpy(y)), err_flag=err)
    sync()
    assert int(err) == 0
    return dict(zip(Cal.STATE_FIELDS, state.cpu().tolist())), state


def test_fit_against_the_float64_reference_and_its_scaling(L):
    z, y = make_logits(11, 300, 5, scale=4.0, p_right=0.6)
    got = {}
    for s in (1.0, 2.0):  # (a power of two: the scaled float32 logits are exact)
        zs = (z * np.float32(s)).astype(np.float32)
        st, raw = fit_on_device(zs, y)
        ref = CR.fit(zs, y)
        tol = CR.fit_tolerance(zs, y, ref["u"])
        print(f"fit x{s}: u {st['u']:.12f} ref {ref['u']:.12f} err / tol {abs(st['u'] - ref['u']) / tol:.4f}")
        assert ref["at_bound"] == 0 and st["at_bound"] == 0 and st["iteration"] == CR.FIT_ITERS
        assert abs(st["u"] - ref["u"]) <= tol
        assert st["u"] in (st["lo"], st["hi"]) and math.log(st["hi"] / st["lo"]) <= CR.RESOLUTION * (1 + 1e-6)
        # nll and g are those of the u the fit returns, nll_at_1 those of u = 1
        b, b1 = CR.bounds(zs, y, st["u"]), CR.bounds(zs, y, 1.0)
        assert abs(st["nll"] - CR.moments(zs, y, st["u"])[0]) <= b["nll_sum"]
        assert abs(st["g"] - CR.moments(zs, y, st["u"])[1]) <= b["g_sum"]
        assert abs(st["nll_at_1"] - CR.moments(zs, y, 1.0)[0]) <= b1["nll_sum"]
        assert st["nll"] <= st["nll_at_1"]
        assert torch.equal(raw.view(torch.int64), fit_on_device(zs, y)[1].view(torch.int64)), "a fit is bit-reproducible"
        got[s] = (st["u"], tol)
    # scaling the logits by s scales T = 1 / u by s
    assert abs(2.0 * got[2.0][0] - got[1.0][0]) <= got[1.0][1] + 2.0 * got[2.0][1]


def test_fit_ends_at_its_bounds(L):
    rng = np.random.default_rng(5)
    z = rng.normal(size=(50, 6)).astype(np.float32)
    y = rng.integers(0, 6, 50).astype(np.int64)
    right, wrong = z.copy(), z.copy()
    right[np.arange(50), y] += 60.0
    wrong[np.arange(50), y] -= 60.0
    st, _ = fit_on_device(right, y)
    assert (st["u"], st["at_bound"], st["iteration"]) == (CR.U_MAX, 1.0, 3.0) == tuple(CR.fit(right, y)[k] for k in ("u", "at_bound", "iteration"))
    assert abs(st["nll"] - CR.moments(right, y, CR.U_MAX)[0]) <= CR.bounds(right, y, CR.U_MAX)["nll_sum"]
    st, _ = fit_on_device(wrong, y)
    assert (st["u"], st["at_bound"], st["iteration"]) == (CR.U_MIN, -1.0, 2.0) == tuple(CR.fit(wrong, y)[k] for k in ("u", "at_bound", "iteration"))
    assert abs(st["nll"] - CR.moments(wrong, y, CR.U_MIN)[0]) <= CR.bounds(wrong, y, CR.U_MIN)["nll_sum"]


# ------------------------------------------------------------------------------------------------------------- ss_calib_bins
def centre_rows(C, n_bins, u=1.0):
    """For every bin whose centre lies above 1 / C: rows [a / u, 0, ..., 0] (confidence at the centre under inverse temperature u)
    with the labels 0 (a hit, rank 0) and, where they exist, 1, 3 and C - 1: label y ranks y -- class 0 is larger, the zeros
    below y tie and come first, the zeros above y tie and do not count."""
    rows, labels = [], []
    for j in range(n_bins):
        if (j + 0.5) / n_bins <= 1.0 / C:
            continue
        row = CR.bin_centre_rows(C, n_bins, j)
        row[0] = np.float32(row[0] / u)
        for lab in sorted({0, min(1, C - 1), min(3, C - 1), C - 1}):
            rows.append(row)
            labels.append(lab)
    return np.stack(rows), np.array(labels, np.int64)


def run_bins(L, z, y, u, n_bins, k_max):
    from silent_speech_amd import calibrate as Cal

    inv = None if u is None else torch.full((1,), u, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = Cal.reliability(cuda(torch.from_numpy(z)), cuda(torch.from_numpy(y)), inv, n_bins, k_max, err_flag=err)
    sync()
    return [t.cpu().numpy() for t in out], int(err)


def check_bins(L, z, y, u, n_bins, k_max, what):
    (cnt, hits, fx, rank), flag = run_bins(L, z, y, u, n_bins, k_max)
    uu = 1.0 if u is None else u
    ref = CR.bins(z, y, uu, n_bins, k_max)
    ok = CR.counts(y, z.shape[1])
    assert abs(ref["conf"][ok] * n_bins - np.floor(ref["conf"][ok] * n_bins) - 0.5).max() < 1e-3 or n_bins == 1, "rows sit at bin centres"
    assert cnt.tolist() == ref["bin_count"].tolist() and hits.tolist() == ref["bin_hits"].tolist(), what
    assert rank.tolist() == ref["rank_hist"].tolist() and len(rank) == k_max + 1, what
    tol = int(ok.sum()) * 2.0 ** 32 * float(CR.bounds(z, np.where(ok, y, 0), uu)["conf"].max())
    worst = float(np.abs(fx.astype(np.float64) - ref["bin_conf"] * 2.0 ** 32).max())
    print(f"bins {what}: conf_fx err / bound {worst / tol:.5f}")
    assert worst <= tol, what
    return flag


@pytest.mark.parametrize("C", [2, 10, 100])
@pytest.mark.parametrize("n_bins", [10, 15])
def test_bins_on_rows_at_the_bin_centres(L, C, n_bins):
    z, y = centre_rows(C, n_bins)
    assert check_bins(L, z, y, None, n_bins, 5, f"C={C} n_bins={n_bins}") == 0
    if C == 10:  # the device float: the same confidences from logits stretched by 1 / u, and the hits and ranks of u = 1
        z2, y2 = centre_rows(C, n_bins, u=0.5)
        assert check_bins(L, z2, y2, 0.5, n_bins, 5, f"C={C} n_bins={n_bins} u=0.5") == 0


def test_bins_edge_sizes_ties_and_bad_labels(L):
    z, y = centre_rows(10, 15)
    for n_bins, k_max in ((15, 1), (15, 10), (1, 5), (64, 64)):
        if n_bins == 64:
            z, y = centre_rows(10, 64)
        assert check_bins(L, z, y, None, n_bins, k_max, f"n_bins={n_bins} k_max={k_max}") == 0
    # ties on both sides of y, equal maxima (the lowest index predicts), rows of all-equal logits
    zt = np.float32([[1, 1, 1, 1], [2, 5, 2, 5], [2, 5, 2, 5], [2, 5, 2, 5], [0, -1, 3, 3], [3, 3, 0, -1]])
    yt = np.int64([2, 3, 1, 2, 0, 1])
    (cnt, hits, fx, rank), flag = run_bins(L, zt, yt, None, 4, 2)
    ref = CR.bins(zt, yt, 1.0, 4, 2)
    assert flag == 0 and rank.tolist() == ref["rank_hist"].tolist() == [1, 2, 3]
    assert cnt.tolist() == ref["bin_count"].tolist() and hits.tolist() == ref["bin_hits"].tolist() and hits.sum() == 1
    # labels outside the classes: first, middle and last row count nowhere, the flag is raised
    z, y = centre_rows(10, 15)
    bad = y.copy()
    bad[0], bad[len(y) // 2], bad[-1] = -1, 10, 2 ** 33 + 1
    assert check_bins(L, z, bad, None, 15, 5, "bad labels") == 1
    lib = L.load()
    for n_bins, k_max in ((0, 5), (65, 5), (15, 0), (15, 65)):
        assert lib.ss_calib_bins(8, 8, 4, 3, None, n_bins, k_max, 8, 8, 8, 8, 8, None) == -1


# ---------------------------------------------------------------------------------------------------------- ss_softmax_topk_t
def run_topk(L, x_d, k, inv):
    """inv: "plain" = ss_softmax_topk, None = ss_softmax_topk_t with NULL, a float = with that device float."""
    B, C = x_d.shape
    probs = torch.full((B, k), 7.0, device="cuda")
    idx = torch.full((B, k), 7, device="cuda", dtype=torch.int32)
    if inv == "plain":
        L.call("ss_softmax_topk", x_d.data_ptr(), B, C, k, probs.data_ptr(), idx.data_ptr(), L.stream())
    else:
        inv_d = None if inv is None else torch.full((1,), inv, dtype=torch.float32, device="cuda")
        L.call("ss_softmax_topk_t", x_d.data_ptr(), B, C, k, L.ptr(inv_d), probs.data_ptr(), idx.data_ptr(), L.stream())
    sync()
    return probs.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("C", [1, 2, 64, 65])
def test_softmax_topk_t(L, C):
    rng = np.random.default_rng(C)
    x = (3.0 * rng.normal(size=(5, C))).astype(np.float32)
    if C > 2:
        x[1, 1] = x[1, 0]          # a tie: the lower index first
        x[2, :] = 0.25             # a whole row of equal logits
    x_d = cuda(torch.from_numpy(x))
    for k in sorted({1, 3, min(C, 64)}):  # (k = C, as far as both kernels take it: k = 65 is refused, below)
        p0, i0 = run_topk(L, x_d, k, "plain")
        for inv in (None, 1.0):    # NULL and a stored 1.0f: the bits of ss_softmax_topk
            p, i = run_topk(L, x_d, k, inv)
            assert p.tobytes() == p0.tobytes() and i.tobytes() == i0.tobytes(), (C, k, inv)
        for u in (0.5, 3.0):
            p, i = run_topk(L, x_d, k, u)
            assert i.tobytes() == i0.tobytes(), "the indices do not depend on the temperature"
            want, bound = CR.softmax_bound(x, u)
            worst = 0.0
            for b in range(5):
                for j in range(k):
                    if i0[b, j] < 0:
                        assert j >= C and p[b, j] == 0.0
                        continue
                    err, tol = abs(float(p[b, j]) - want[b, i0[b, j]]), bound[b, i0[b, j]]
                    worst = max(worst, err / tol)
                    assert err <= tol, (C, k, u, b, j, err, tol)
            print(f"softmax_topk_t C={C} k={k} u={u}: largest err / bound {worst:.4f}")
    lib = L.load()
    assert lib.ss_softmax_topk_t(x_d.data_ptr(), 5, C, 65, None, 8, 8, None) == -3  # as ss_softmax_topk refuses it:
    assert lib.ss_softmax_topk(x_d.data_ptr(), 5, C, 65, 8, 8, None) == -3


# --------------------------------------------------------------------------------------------------------------- launch lists
def test_launch_lists_with_and_without_a_temperature(ss):
    from silent_speech_amd.checkpoint import softmax_topk

    mp = pytest.MonkeyPatch()
    nobody = types.SimpleNamespace(_ws_cache={})
    logits = torch.randn(6, 5, generator=torch.Generator().manual_seed(2)).cuda()
    plain = LT.traced(mp, nobody, lambda: softmax_topk(logits, 3))
    assert plain == [["launch", "ss_softmax_topk", "ss_softmax_topk", "main", ["ptr", 6, 5, 3, "ptr", "ptr"]]]
    tempered = LT.traced(mp, nobody, lambda: softmax_topk(logits, 3, temperature=2.0))
    assert tempered == [["launch", "ss_softmax_topk_t", "ss_softmax_topk_t", "main", ["ptr", 6, 5, 3, "ptr", "ptr", "ptr"]]]
    p0, i0 = softmax_topk(logits, 3)
    p1, i1 = softmax_topk(logits, 3, temperature=1.0)
    p2, i2 = softmax_topk(logits, 3, temperature=2.0)
    assert torch.equal(p0, p1) and torch.equal(i0, i1) and torch.equal(i0, i2) and not torch.equal(p0, p2)
    want = torch.softmax(logits.double() / 2.0, 1).gather(1, i0.long())
    assert float((p2.double() - want).abs().max()) < 1e-6
    assert ss.topk_from_logits(logits[:1], {i: str(i) for i in range(5)}, temperature=2.0) == \
        [(str(int(i)), float(p)) for p, i in zip(p2[0].cpu(), i2[0].cpu())]

    # the captured serving graph: without a temperature every launch of today's; with one, only the top-k entry differs
    model = ss.BiGRUClassifier(84, 5).cuda().eval()
    B, T = 4, 6
    made = {}
    t_plain = LT.launches(LT.traced(mp, model, lambda: made.update(plain=ss.GraphedInference(model, B, T, topk=3))))
    t_temp = LT.launches(LT.traced(mp, model, lambda: made.update(temp=ss.GraphedInference(model, B, T, topk=3, temperature=1.0))))
    names = [e[1] for e in t_plain]
    assert names.count("ss_softmax_topk") == 3 and "ss_softmax_topk_t" not in names  # two warm-up runs and the capture
    assert t_plain[-1][:3] == ["launch", "ss_softmax_topk", "ss_softmax_topk"] and t_plain[-1][4] == ["ptr", B, 5, 3, "ptr", "ptr"]
    assert len(t_temp) == len(t_plain)
    for a, b in zip(t_plain, t_temp):
        if a[1] == "ss_softmax_topk":
            assert b == ["launch", "ss_softmax_topk_t", "ss_softmax_topk_t", a[3], a[4][:4] + ["ptr"] + a[4][4:]]
        else:
            assert a == b
    # replays: T = 1 gives the untempered bits; set_temperature changes the next replay's probabilities without a launch
    g0, g1 = made["plain"], made["temp"]
    X = torch.randn(B, T, 84, generator=torch.Generator().manual_seed(3)).cuda()
    out0 = g0(X).clone()
    out1 = g1(X).clone()
    assert torch.equal(out0, out1) and torch.equal(g0.top_probs, g1.top_probs) and torch.equal(g0.top_idx, g1.top_idx)
    g1.set_temperature(2.5)
    replay = LT.traced(mp, model, lambda: g1(X))
    assert LT.launches(replay) == []
    sync()
    want_p, want_i = softmax_topk(out1, 3, temperature=2.5)
    assert torch.equal(g1.top_probs, want_p) and torch.equal(g1.top_idx, want_i) and not torch.equal(g1.top_probs, g0.top_probs)
    with pytest.raises(RuntimeError, match="set_temperature"):
        g0.set_temperature(2.0)
    with pytest.raises(ValueError, match="temperature"):
        g1.set_temperature(0.0)


# ----------------------------------------------------------------------------------------------------------------- end to end
FIT = dict(epochs=3, batch_size=16, patience=3, max_t=24, lr=3e-3, plan="device")


def same_weights(a, b):
    return list(a["model"]) == list(b["model"]) and \
        all(torch.equal(a["model"][k].view(torch.int32), b["model"][k].view(torch.int32)) for k in a["model"])


def test_fit_with_calibrate_end_to_end(ss, tmp_path, monkeypatch):
    """``fit_calibrated`` against the files ``fit`` writes, weights bit for bit.  Two training runs of one seed do not give equal
    bits in this project (the training kernels add with float atomics: LOSS_BOUND in test_gpu_ema_resume.py), so a second,
    separately trained checkpoint cannot be the yardstick.  The comparison is made twice where it is exact: (1) against the file
    the calibrated run itself had written when training was over, read just before calibration rewrites it; (2) a plain ``fit``
    run's file, calibrated afterwards by a ``fit_calibrated`` call on the finished run, against that file as ``fit`` left it."""
    from silent_speech_amd import harness as Hn

    clip_dir = write_clips(str(tmp_path / "clips_npz"), WORDS)
    plain, cal = str(tmp_path / "plain.pt"), str(tmp_path / "cal.pt")
    plain_state, state = str(tmp_path / "plain_state.pt"), str(tmp_path / "cal_state.pt")
    old_keys = {"model", "x_dim", "max_t", "use_roi", "roi_w", "roi_h", "labels", "label_to_id", "id_to_label", "seed", "gru_layers"}
    seen, real = [], Hn.calibrate_checkpoint

    def spy(out_path, *args, **kw):
        seen.append(torch.load(out_path, weights_only=False))  # the file as training left it
        return real(out_path, *args, **kw)

    monkeypatch.setattr(Hn, "calibrate_checkpoint", spy)
    # (1) calibration at the end of a run
    logs = []
    best_cal = Hn.fit_calibrated(clip_dir, cal, state_path=state, log=logs.append, **FIT)
    assert len(seen) == 1 and set(seen[0]) == old_keys
    b = torch.load(cal, weights_only=False)
    assert set(b) == old_keys | {"temperature", "calibration"}
    assert same_weights(seen[0], b) and all(seen[0][k] == b[k] for k in old_keys - {"model"})
    c = b["calibration"]
    assert isinstance(b["temperature"], float) and b["temperature"] == c["temperature"]
    assert 1.0 / CR.U_MAX <= b["temperature"] <= 1.0 / CR.U_MIN
    assert c["nll_after"] <= c["nll_before"]
    assert c["n"] == sum(c["bin_count_before"]) == sum(c["bin_count_after"]) > 0
    assert len(c["topk_acc"]) == 5 and c["topk_acc"][0] == best_cal and c["topk_acc"][2] == 1.0  # three words: top-3 is everything
    assert sum("calibrated" in str(m) and "ECE" in str(m) for m in logs) == 1
    model = ss.load_classifier(cal)[0]
    assert model.temperature == b["temperature"]
    # a second call on the finished run reproduces the temperature bit for bit
    logs2 = []
    assert Hn.fit_calibrated(clip_dir, cal, state_path=state, resume=True, log=logs2.append, **FIT) == best_cal
    again = torch.load(cal, weights_only=False)
    assert again["temperature"] == b["temperature"] and again["calibration"] == c and same_weights(b, again)
    assert any("Nothing to resume" in str(m) for m in logs2) and sum("calibrated" in str(m) for m in logs2) == 1
    # (2) a run without calibration: today's keys; calibrated afterwards, the weights are the bits that run wrote
    best_plain = Hn.fit(clip_dir, plain, state_path=plain_state, log=lambda *a: None, **FIT)
    a = torch.load(plain, weights_only=False)
    assert len(seen) == 2 and set(a) == old_keys and ss.load_classifier(plain)[0].temperature == 1.0
    assert Hn.fit_calibrated(clip_dir, plain, state_path=plain_state, resume=True, log=lambda *a: None, **FIT) == best_plain
    a2 = torch.load(plain, weights_only=False)
    assert len(seen) == 3 and set(a2) == old_keys | {"temperature", "calibration"}
    assert same_weights(a, a2) and all(a[k] == a2[k] for k in old_keys - {"model"})
    assert a2["calibration"]["nll_after"] <= a2["calibration"]["nll_before"]
    # the standalone call gives the same figures from the same weights
    from silent_speech_amd.calibrate import calibrate as run_calibration

    info = Hn.scan_clips(clip_dir)
    _, val_files = Hn.split_by_label(info["files"], info["labels"], Hn.VAL_FRAC, seed=Hn.SEED)
    store = ss.DeviceClipStore(val_files, info["label_to_id"], max_t=24, use_roi=True)
    assert run_calibration(model, store, 16).plain() == c
