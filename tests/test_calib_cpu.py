"""CPU: ``calib_ref`` (the float64 restatement of csrc/calib.hip) pinned against torch and against its own properties, the host
arithmetic of ``silent_speech_amd.calibrate`` (ECE, MCE, top-k from the device's integers), and the host-only side of the new
arguments: the ``ValueError``s, the checkpoint keys present and absent, ``model.temperature``, the header's constants."""
import math
import os
import re

import numpy as np
import pytest
import torch

import calib_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_logits(seed, N, C, scale=3.0, p_right=0.7):
    """Random logits whose arg-max is the label with probability ``p_right``."""
    rng = np.random.default_rng(seed)
    z = (scale * rng.normal(size=(N, C))).astype(np.float32)
    y = np.where(rng.random(N) < p_right, z.argmax(1), rng.integers(0, C, N)).astype(np.int64)
    return z, y


# ------------------------------------------------------------------------------------------------------------ row values
@pytest.mark.parametrize("C,u", [(2, 1.0), (3, 0.37), (65, 2.5), (130, 0.05), (7, 20.0)])
def test_row_values_against_log_softmax_and_autograd(C, u):
    z, y = make_logits(C, 9, C)
    zt = torch.from_numpy(z).double()
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    nll_t = -torch.log_softmax(ut * zt, 1)[torch.arange(len(y)), torch.from_numpy(y)]
    nll, g, ok = CR.row_values(z, y, u)
    assert ok.all()
    np.testing.assert_allclose(nll, nll_t.detach().numpy(), rtol=1e-12, atol=1e-12)
    for i in range(len(y)):
        (gi,) = torch.autograd.grad(nll_t[i], ut, retain_graph=True)
        assert abs(g[i] - float(gi)) <= 1e-12 * max(1.0, abs(float(gi)))
    s_nll, s_g = CR.moments(z, y, u)
    assert abs(s_nll - float(nll_t.detach().sum())) <= 1e-11 * abs(float(nll_t.detach().sum()))
    # the slope of sum g: a central difference of sum g against the second moment
    h = 1e-5 * u
    slope = (CR.moments(z, y, u + h)[1] - CR.moments(z, y, u - h)[1]) / (2 * h)
    assert abs(slope - CR.second_moment(z, y, u)) <= 1e-6 * max(1.0, abs(slope))


def test_rows_with_a_label_outside_the_classes_count_nowhere():
    z, y = make_logits(1, 6, 4)
    y_bad = y.copy()
    y_bad[[0, 3, 5]] = [-1, 4, 2 ** 40]
    keep = [1, 2, 4]
    assert CR.moments(z, y_bad, 0.8) == pytest.approx(CR.moments(z[keep], y[keep], 0.8), rel=1e-14)
    assert CR.ranks(z, y_bad)[[0, 3, 5]].tolist() == [-1, -1, -1]
    b, want = CR.bins(z, y_bad, 1.0, 5, 3), CR.bins(z[keep], y[keep], 1.0, 5, 3)
    for k in ("bin_count", "bin_hits", "rank_hist"):
        assert b[k].tolist() == want[k].tolist()
    assert b["bin_count"].sum() == 3


# ------------------------------------------------------------------------------------------------------------------ the fit
def test_fit_against_a_dense_grid_search():
    z, y = make_logits(3, 400, 5, scale=4.0, p_right=0.6)
    st = CR.fit(z, y)
    assert st["at_bound"] == 0 and st["iteration"] == CR.FIT_ITERS and CR.U_MIN < st["lo"] <= st["hi"] < CR.U_MAX
    assert st["u"] in (st["lo"], st["hi"]) and math.log(st["hi"] / st["lo"]) <= CR.RESOLUTION * (1 + 1e-6)
    assert st["nll"] == CR.moments(z, y, st["u"])[0] and st["nll_at_1"] == CR.moments(z, y, 1.0)[0]
    grid = np.exp(np.linspace(math.log(CR.U_MIN), math.log(CR.U_MAX), 6001))
    best = grid[int(np.argmin([CR.moments(z, y, float(u))[0] for u in grid]))]
    spacing = math.log(CR.U_MAX / CR.U_MIN) / 6000
    assert abs(math.log(st["u"] / best)) <= spacing
    assert st["nll"] <= st["nll_at_1"]
    assert abs(st["g"]) <= 2 * st["u"] * CR.RESOLUTION * CR.second_moment(z, y, st["u"]) + 1e-9


@pytest.mark.parametrize("s", [0.5, 2.0, 3.0])
def test_scaling_the_logits_scales_the_temperature(s):
    z, y = make_logits(4, 300, 4, scale=2.0, p_right=0.65)
    u1 = CR.fit(z, y)["u"]
    us = CR.fit(z.astype(np.float64) * s, y)["u"]
    # T = 1 / u scales by s; both fits are ends of brackets of width RESOLUTION in ln u around their roots
    assert abs(math.log((1.0 / us) / (s / u1))) <= 2 * CR.RESOLUTION + 1e-12


def test_logits_calibrated_by_construction_give_temperature_one():
    # every distinct row appears with its labels in exactly the proportions its softmax claims: sum g vanishes at u = 1
    rows, labels = [], []
    for zrow, counts in (([math.log(3.0), 0.0], (3, 1)), ([0.0, math.log(4.0)], (1, 4)), ([0.0, 0.0], (1, 1))):
        for c, k in enumerate(counts):
            rows += [zrow] * k
            labels += [c] * k
    z, y = np.array(rows), np.array(labels)
    assert abs(CR.moments(z, y, 1.0)[1]) < 1e-14
    st = CR.fit(z, y)
    assert st["at_bound"] == 0 and abs(math.log(st["u"])) <= 2 * CR.RESOLUTION


def test_fit_ends_at_the_bounds():
    rng = np.random.default_rng(5)
    z = rng.normal(size=(50, 6))
    y = rng.integers(0, 6, 50)
    right = z.copy()
    right[np.arange(50), y] += 60.0   # all correct, large margins: the likelihood keeps growing with u
    st = CR.fit(right, y)
    assert st["at_bound"] == 1 and st["u"] == CR.U_MAX and st["iteration"] == 3
    assert st["nll"] == CR.moments(right, y, CR.U_MAX)[0]
    wrong = z.copy()
    wrong[np.arange(50), y] -= 60.0   # all wrong: the flatter the better
    st = CR.fit(wrong, y)
    assert st["at_bound"] == -1 and st["u"] == CR.U_MIN and st["iteration"] == 2
    assert st["nll"] == CR.moments(wrong, y, CR.U_MIN)[0]


# ----------------------------------------------------------------------------------------------------------- bins and ranks
def test_ece_is_zero_where_every_bin_hits_its_confidence():
    from silent_speech_amd import calibrate as Cal

    rows, labels = [], []
    for zrow, hits, misses in (([math.log(3.0), 0.0], 3, 1), ([0.0, 0.0], 1, 1), ([math.log(9.0), 0.0], 9, 1)):
        rows += [zrow] * (hits + misses)
        labels += [0] * hits + [1] * misses
    b = CR.bins(np.array(rows), np.array(labels), 1.0, n_bins=10, k_max=2)
    assert b["bin_count"].tolist() == [0, 0, 0, 0, 0, 2, 0, 4, 0, 10] and b["bin_hits"].tolist() == [0, 0, 0, 0, 0, 1, 0, 3, 0, 9]
    ece, mce = CR.ece_mce(b["bin_count"], b["bin_hits"], b["bin_conf"])
    assert ece < 1e-15 and mce < 1e-15
    # the host arithmetic of the package on the integers the device would hand over: exactly zero
    fx = [0, 0, 0, 0, 0, 2 ** 32, 0, 3 * 2 ** 32, 0, 9 * 2 ** 32]
    acc, conf, ece, mce = Cal.bin_stats(b["bin_count"], b["bin_hits"], fx)
    assert ece == 0.0 and mce == 0.0 and acc[7] == 0.75 == conf[7] and acc[0] == 0.0
    # and a set that is off by a known amount: two clips at confidence 0.75, none right
    acc, conf, ece, mce = Cal.bin_stats([0, 0, 2, 0], [0, 0, 0, 0], [0, 0, 3 * 2 ** 31, 0])
    assert ece == 0.75 and mce == 0.75
    assert Cal.topk_accuracy([6, 2, 1, 1]) == [0.6, 0.8, 0.9]


def test_rank_rule_with_ties():
    z = np.array([[1.0, 1.0, 1.0, 1.0],    # all equal: the rank of y is y
                  [2.0, 5.0, 2.0, 5.0],    # y = 3 ties with class 1 below it
                  [2.0, 5.0, 2.0, 5.0],    # y = 1: the tie at class 3 is above y and does not count
                  [2.0, 5.0, 2.0, 5.0],    # y = 2: two larger, one equal below
                  [0.0, -1.0, 3.0, 3.0]])
    y = np.array([2, 3, 1, 2, 0])
    assert CR.ranks(z, y).tolist() == [2, 1, 0, 3, 2]
    b = CR.bins(z, y, 1.0, n_bins=4, k_max=2)
    assert b["rank_hist"].tolist() == [1, 1, 3] and b["pred"].tolist() == [0, 1, 1, 1, 2]
    assert b["bin_hits"].sum() == 1  # only row 2 is predicted right: rank 0 <=> hit


def test_bin_centre_rows_land_in_their_bins():
    for C in (2, 10, 100):
        for n_bins in (10, 15):
            for j in range(n_bins):
                if (j + 0.5) / n_bins <= 1.0 / C:
                    continue
                row = CR.bin_centre_rows(C, n_bins, j)[None, :]
                conf = float(CR.bins(row, [0], 1.0, n_bins, 1)["conf"][0])
                assert abs(conf * n_bins - (j + 0.5)) < 1e-3


def test_bounds_are_small_positive_and_grow_with_the_row():
    z, y = make_logits(8, 40, 65)
    b = CR.bounds(z, y, 1.3)
    nll, g = CR.moments(z, y, 1.3)
    assert 0 < b["nll_sum"] < 1e-4 * abs(nll) and 0 < b["g_sum"] < 1e-3 * max(1.0, abs(g)) and (b["conf"] > 0).all()
    assert CR.bounds(z, y, 1.3)["g_sum"] < CR.bounds(np.concatenate([z, z]), np.concatenate([y, y]), 1.3)["g_sum"]


# ------------------------------------------------------------------------------------------------------------- host checks
def test_constants_and_prototypes_agree_with_the_header():
    from silent_speech_amd import _lib
    from silent_speech_amd import calibrate as Cal

    hdr = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    define = lambda name: float(re.search(rf"#define {name} (\S+)", hdr).group(1))  # noqa: E731
    assert (define("SS_CALIB_U_MIN"), define("SS_CALIB_U_MAX")) == (Cal.U_MIN, Cal.U_MAX) == (CR.U_MIN, CR.U_MAX)
    assert define("SS_CALIB_FIT_ITERS") == Cal.FIT_ITERS == CR.FIT_ITERS == 3 + 32
    assert define("SS_CALIB_MAX_PARTIALS") == Cal.MAX_PARTIALS
    assert [Cal.n_partials_for(n) for n in (1, 4, 5, 4 * Cal.MAX_PARTIALS, 10 ** 6)] == [1, 1, 2, Cal.MAX_PARTIALS, Cal.MAX_PARTIALS]
    lib = _lib.load()
    for name, n_args in (("ss_calib_moments", 9), ("ss_calib_bisect", 4), ("ss_calib_bins", 13), ("ss_softmax_topk_t", 8)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == n_args
        decl = re.search(rf"int {name}\((.*?)\);", hdr, flags=re.S)
        assert len(decl.group(1).split(",")) == n_args
    assert len(_lib.SIGNATURES["ss_softmax_topk_t"]) == len(_lib.SIGNATURES["ss_softmax_topk"]) + 1
    assert lib.ss_abi_version() == 3
    # every SS_ERR_ARG case returns before a launch (no device here: a launch would fail differently)
    assert lib.ss_calib_moments(8, 8, 4, 1, 8, 8, 1, 8, None) == -1          # one class
    assert lib.ss_calib_moments(8, 8, 4, 3, 8, 8, Cal.MAX_PARTIALS + 1, 8, None) == -1
    assert lib.ss_calib_moments(8, 8, 0, 3, 8, 8, 1, 8, None) == -1
    assert lib.ss_calib_bisect(8, 8, 0, None) == -1 and lib.ss_calib_bisect(None, 8, 1, None) == -1
    for n_bins, k_max in ((0, 5), (65, 5), (15, 0), (15, 65)):
        assert lib.ss_calib_bins(8, 8, 4, 3, None, n_bins, k_max, 8, 8, 8, 8, 8, None) == -1
    assert lib.ss_softmax_topk_t(8, 2, 3, 65, None, 8, 8, None) == -3 and lib.ss_softmax_topk_t(8, 0, 3, 1, None, 8, 8, None) == -1


@pytest.mark.parametrize("bad", [0, 0.0, -1.5, float("inf"), float("nan"), "2", True, 1e-60, 1e60, [2.0]])
def test_a_temperature_that_is_no_positive_finite_number_is_refused_on_the_host(bad):
    import silent_speech_amd as ss
    from silent_speech_amd.checkpoint import softmax_topk

    logits = torch.zeros(2, 3)  # a CPU tensor: the temperature is looked at before anything else
    with pytest.raises(ValueError, match="temperature"):
        softmax_topk(logits, 2, temperature=bad)
    with pytest.raises(ValueError, match="temperature"):
        ss.topk_from_logits(logits[:1], {0: "a", 1: "b", 2: "c"}, temperature=bad)
    m = ss.BiGRUClassifier(20, 3)
    with pytest.raises(ValueError, match="temperature"):
        ss.GraphedInference(m, 2, 4, topk=2, temperature=bad)
    with pytest.raises(ValueError, match="temperature"):
        ss.save_checkpoint("unused.pt", m, ["a", "b", "c"], temperature=bad)


def test_good_temperatures_pass_and_none_keeps_the_old_refusal():
    from silent_speech_amd import calibrate as Cal
    from silent_speech_amd.checkpoint import softmax_topk

    assert Cal.check_temperature(2) == 2.0 and Cal.check_temperature(np.float32(0.5)) == 0.5
    for call in (lambda: softmax_topk(torch.zeros(2, 3), 2), lambda: softmax_topk(torch.zeros(2, 3), 2, temperature=1.5)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for n_bins, k_max in ((0, 5), (65, 5), (15, 0), (15, 65), (15.0, 5), (True, 5)):
        with pytest.raises(ValueError):
            Cal.check_bins(n_bins, k_max)
    assert Cal.check_bins(1, 64) == (1, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        Cal.fit_temperature(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))


def test_checkpoint_keys_present_and_absent(tmp_path):
    import silent_speech_amd as ss
    from silent_speech_amd import calibrate as Cal
    from silent_speech_amd.checkpoint import add_calibration

    m = ss.BiGRUClassifier(20, 3)
    plain, cal_path = str(tmp_path / "plain.pt"), str(tmp_path / "cal.pt")
    ss.save_checkpoint(plain, m, ["a", "b", "c"])
    old_keys = {"model", "x_dim", "max_t", "use_roi", "roi_w", "roi_h", "labels", "label_to_id", "id_to_label", "seed", "gru_layers"}
    assert set(torch.load(plain, weights_only=False)) == old_keys
    cal = Cal.calibration_from_host([0.5, 0.4, 0.6, 12.0, 0.0, 16.0, 35.0, 0.0], ([0, 4], [0, 3], [0, 3 * 2 ** 32]),
                                    ([1, 3], [0, 3], [2 ** 31, 3 * 2 ** 32]), [3, 1, 0])
    assert cal.temperature == 2.0 and cal.n == 4 and cal.nll_before == 4.0 and cal.nll_after == 3.0 and cal.at_bound == 0
    assert cal.ece_before == 0.0 and cal.ece_after == pytest.approx(0.125) and cal.mce_after == 0.5 and cal.topk_acc == [0.75, 1.0]
    ss.save_checkpoint(cal_path, m, ["a", "b", "c"], temperature=cal.temperature, calibration=cal.plain())
    ckpt = torch.load(cal_path, weights_only=False)
    assert set(ckpt) == old_keys | {"temperature", "calibration"}
    assert ckpt["temperature"] == 2.0 and isinstance(ckpt["temperature"], float) and ckpt["calibration"] == cal.plain()
    assert all(isinstance(v, (int, float, list)) for v in ckpt["calibration"].values())
    with pytest.raises(ValueError, match="calibration"):
        ss.save_checkpoint(cal_path, m, ["a", "b", "c"], calibration=[1, 2])
    # load_classifier: the same 4-tuple, the temperature as a plain attribute, the state_dict keys where they were
    for path, want in ((plain, 1.0), (cal_path, 2.0)):
        out = ss.load_classifier(path, device="cpu")
        assert len(out) == 4 and out[0].temperature == want and isinstance(out[0].temperature, float)
        assert list(out[0].state_dict()) == list(m.state_dict())
    # add_calibration: the two keys added to an existing file, everything else and the weights' bits as they were
    add_calibration(plain, 1.25, cal.plain())
    again, first = torch.load(plain, weights_only=False), torch.load(cal_path, weights_only=False)
    assert set(again) == old_keys | {"temperature", "calibration"} and again["temperature"] == 1.25
    assert all(torch.equal(again["model"][k].view(torch.int32), first["model"][k].view(torch.int32)) for k in first["model"])
    assert all(again[k] == first[k] for k in old_keys - {"model"})
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]


def test_fit_calibrated_checks_its_arguments_before_any_work_and_leaves_fit_alone(tmp_path):
    import inspect

    from silent_speech_amd import harness as Hn

    with pytest.raises(TypeError, match="no_such_argument"):  # (before the clip directory, which does not exist, is looked at)
        Hn.fit_calibrated(str(tmp_path / "no_such_dir"), str(tmp_path / "m.pt"), no_such_argument=1)
    with pytest.raises(RuntimeError, match="No .npz files"):  # fit's own refusal passes through
        Hn.fit_calibrated(str(tmp_path / "no_such_dir"), str(tmp_path / "m.pt"), plan="device")
    assert "calibrate" not in inspect.signature(Hn.fit).parameters
    assert Hn.calibrate_checkpoint(str(tmp_path / "missing.pt"), None) is None
