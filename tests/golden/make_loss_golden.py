#!/usr/bin/env python3
"""Record what the nine loss entry points write -- ss_tail_fwd, ss_tail_fwd_w, ss_tail_fwd_mix, ss_ce_ls_fwd_bwd, ss_ce_ls_w_fwd_bwd,
ss_ce_ls_mix_fwd_bwd, ss_eval_accum, ss_eval_accum_w, ss_class_weight_sum -- for a fixed set of small inputs, on one MI355X:

    python tests/golden/make_loss_golden.py tests/golden/loss_bits.npz

Everything goes through the C ABI, so the same ``record()`` runs on any commit; tests/test_gpu_loss_bits.py calls it again and
compares bit for bit.  Inputs come from seeded CPU generators and are not stored.  The fixture's ``header`` entry says which commit
it was recorded on and with what command.

Variants: plain, weighted (w), mix and weighted mix at lam 1.0 and 0.25.  Every label set has one row outside [0, C): the weighted
and the mixed losses and the evaluation skip it (mixed: the bad label is in y_b at lam 1.0 and in y at lam 0.25); the plain loss never looks at a label, so there the row is label -1, which reads
the float in front of the row (the buffers are laid out so that this float exists: a guard float in front of the CE logits, the
last head activation in front of the tail's logit row in LDS).
Sums that float atomics add are a function of the order the waves arrive in.  They are recorded where one wave contributes
(B <= 64 for the CE and evaluation kernels, which here is B = 1; never for the tail, a wave per clip); at larger B every row is run again as a launch of its own, the per-row values are recorded, and the test holds the sum to
the float64 sum of those."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import weights as W  # noqa: E402

EPS = 0.05
I32_MAX = 2 ** 31 - 1
# one lane, a wave boundary, a second workgroup; C < 64 and C > 64.  (Not all nine pairs: d_logits at (65, 100) alone is 26 KB per
# variant, and the row function does not know B.)
CE_SHAPES = ((1, 2), (1, 100), (65, 2), (65, 5), (257, 2))
VARIANTS = (("plain", False, None), ("w", True, None), ("mix_lam1", False, 1.0), ("mix_lam25", False, 0.25),
            ("wmix_lam1", True, 1.0), ("wmix_lam25", True, 0.25))
TAIL = dict(B=3, T=7, lengths=(7, 1, 4), D=128, MID=32)
TAIL_C = (5, 100)
TAIL_DROP = ((0.0, 0), (0.2, 1234))
DROP_OFFSET = 7 << 40


def cuda(t):
    return t.contiguous().cuda()


def make_weights(g, C):
    w = torch.rand(C, generator=g) * 2.8 + 0.2
    return (w / w.mean()).float()


def labels(g, B, C):
    """-> (y, y_b, y with the bad row, y_b with the bad row): y_b a permutation of y's classes; the row in the middle (the only one
    at B = 1: that shape runs a second time with its label inside) is outside the classes: y = -1,
    y_b = C (``mix_labels`` says which of the two a variant gets)."""
    y = torch.randint(0, C, (B,), generator=g)
    y_b = y[torch.randperm(B, generator=g)] if B > 1 else (y + 1) % C
    bad_y, bad_yb = y.clone(), y_b.clone()
    bad_y[B // 2] = -1
    bad_yb[B // 2] = C
    return y, y_b, bad_y, bad_yb


def mix_labels(lam, y_d, yb_d, bad_y_d, bad_yb_d):
    """-> (y, y_b) of a variant with a bad row: one label: in y; two labels: in y_b at lam = 1, in y otherwise, the other vector whole."""
    if lam is None:
        return bad_y_d, bad_yb_d
    return (y_d, bad_yb_d) if lam == 1.0 else (bad_y_d, yb_d)


def ce_inputs(B, C):
    g = torch.Generator().manual_seed(1000 * B + C)
    lg = torch.randn(B, C, generator=g) * 3
    if B >= 3:  # two equal maxima: the arg-max is the lower index
        lg[2, C - 1] = lg[2, C // 2 - (C == 2)] = float(lg[2].max()) + 1.0
    return lg, make_weights(g, C), labels(g, B, C)


def ce_call(L, weighted, lam_d, lg_p, y_p, yb_p, B, C, denom, w_d, den_d, d_p, loss_p, hits_p):
    if lam_d is not None:
        L.call("ss_ce_ls_mix_fwd_bwd", lg_p, y_p, yb_p, lam_d.data_ptr(), B, C, EPS, denom, L.ptr(w_d) if weighted else None,
               L.ptr(den_d) if weighted else None, d_p, loss_p, hits_p, L.stream())
    elif weighted:
        L.call("ss_ce_ls_w_fwd_bwd", lg_p, y_p, B, C, EPS, w_d.data_ptr(), den_d.data_ptr(), d_p, loss_p, hits_p, L.stream())
    else:
        L.call("ss_ce_ls_fwd_bwd", lg_p, y_p, B, C, EPS, denom, d_p, loss_p, hits_p, L.stream())


def record_ce(L, out):
    for B, C in CE_SHAPES:
        lg, w, (y, y_b, bad_y, bad_yb) = ce_inputs(B, C)
        buf = cuda(torch.cat([torch.tensor([0.375]), lg.reshape(-1)]))  # (the guard float in front of row 0)
        lg_p, w_d = buf.data_ptr() + 4, cuda(w)
        label_sets = [("bad", bad_y, bad_yb)] + ([("ok", y, y_b)] if B == 1 else [])
        for tag, ya, yb in label_sets:
            ya_d, yb_d, y_d, ybw_d = cuda(ya), cuda(yb), cuda(y), cuda(y_b)
            den_d = torch.full((1,), -7.0, device="cuda")
            L.call("ss_class_weight_sum", ya_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
            out[f"ce/{B}x{C}/{tag}/den"] = den_d.cpu().numpy()
            for name, weighted, lam in VARIANTS:
                key = f"ce/{B}x{C}/{tag}/{name}"
                lam_d = None if lam is None else torch.tensor([lam], device="cuda")
                first, second = (y_d, ybw_d) if tag == "ok" else mix_labels(lam, y_d, ybw_d, ya_d, yb_d)
                d = torch.full((B, C), 9.0, device="cuda")
                loss, hits = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
                ce_call(L, weighted, lam_d, lg_p, first.data_ptr(), second.data_ptr(), B, C, float(B), w_d, den_d, d.data_ptr(),
                        loss.data_ptr(), hits.data_ptr())
                rows = torch.zeros(B, device="cuda")
                for b in range(B):  # every row as a launch of its own: its term of the sum
                    ce_call(L, weighted, lam_d, lg_p + 4 * b * C, first.data_ptr() + 8 * b, second.data_ptr() + 8 * b, 1, C, float(B),
                            w_d, den_d, None, rows.data_ptr() + 4 * b, None)
                torch.cuda.synchronize()
                out[key + "/d_logits"], out[key + "/hits"] = d.cpu().numpy(), hits.cpu().numpy()
                out[key + "/loss_rows"] = rows.cpu().numpy()
                out[key + ("/loss_sum" if B <= 64 else "/loss_sum_any_order")] = loss.cpu().numpy()
            # the evaluation: both entry points, the same rows
            for name, weighted in (("plain", False), ("w", True)):
                key = f"eval/{B}x{C}/{tag}/{name}"

                def accum(lp, yp, n, first_row, loss_p, wsum_p):
                    st = dict(hits=torch.zeros(1, device="cuda", dtype=torch.int32),
                              confusion=torch.zeros(C, C, device="cuda", dtype=torch.int32),
                              first_seen=torch.full((C, C), I32_MAX, device="cuda", dtype=torch.int32),
                              y_true=torch.full((n,), 77, device="cuda", dtype=torch.int32),
                              y_pred=torch.full((n,), 77, device="cuda", dtype=torch.int32),
                              err_flag=torch.zeros(1, device="cuda", dtype=torch.int32))
                    tail = [st[k].data_ptr() for k in ("hits", "confusion", "first_seen", "y_true", "y_pred", "err_flag")]
                    if weighted:
                        L.call("ss_eval_accum_w", lp, yp, n, C, EPS, first_row, w_d.data_ptr(), loss_p, wsum_p, *tail, L.stream())
                    else:
                        L.call("ss_eval_accum", lp, yp, n, C, EPS, first_row, loss_p, *tail, L.stream())
                    return st

                ye_d = y_d if tag == "ok" else ya_d
                loss, wsum = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
                st = accum(lg_p, ye_d.data_ptr(), B, 1000, loss.data_ptr(), wsum.data_ptr())
                rows, wrows = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
                for b in range(B):
                    accum(lg_p + 4 * b * C, ye_d.data_ptr() + 8 * b, 1, b, rows.data_ptr() + 4 * b, wrows.data_ptr() + 4 * b)
                torch.cuda.synchronize()
                for k, v in st.items():
                    out[f"{key}/{k}"] = v.cpu().numpy()
                out[key + "/loss_rows"] = rows.cpu().numpy()
                sfx = "" if B <= 64 else "_any_order"
                out[key + "/loss_sum" + sfx] = loss.cpu().numpy()
                if weighted:
                    out[key + "/wsum_rows"], out[key + "/wsum" + sfx] = wrows.cpu().numpy(), wsum.cpu().numpy()


def tail_inputs(C):
    B, T, D, MID = TAIL["B"], TAIL["T"], TAIL["D"], TAIL["MID"]
    g = torch.Generator().manual_seed(B * 7 + C)
    sd = W.make_state_dict(31 + C, 84, C, False, hidden=D // 2)
    P = [sd["pool.score.weight"], sd["pool.score.bias"], sd["head.0.weight"], sd["head.0.bias"], sd["head.1.weight"][:MID],
         sd["head.1.bias"][:MID], sd["head.4.weight"][:, :MID], sd["head.4.bias"]]
    h = torch.randn(B, T, D, generator=g)
    for b in range(B):
        h[b, TAIL["lengths"][b]:] = 0
    return P, h, make_weights(g, C), labels(g, B, C)


def tail_call(L, weighted, lam_d, P, h_p, len_p, y_p, yb_p, B, C, drop, offset, denom, w_d, den_d, o):
    T, D, MID = TAIL["T"], TAIL["D"], TAIL["MID"]
    mix = () if lam_d is None else (yb_p, lam_d.data_ptr())
    if lam_d is not None:
        name, norm = "ss_tail_fwd_mix", (denom, w_d.data_ptr() if weighted else None, den_d.data_ptr() if weighted else None)
    elif weighted:
        name, norm = "ss_tail_fwd_w", (w_d.data_ptr(), den_d.data_ptr())
    else:
        name, norm = "ss_tail_fwd", (denom,)
    L.call(name, h_p, len_p, *(p.data_ptr() for p in P), y_p, *mix, B, T, D, MID, C, 1e-5, drop[0], drop[1], offset, EPS, *norm,
           None, None, None, None, None, None, o["logits"].data_ptr(), o["d_logits"].data_ptr(), o["loss"].data_ptr(),
           o["hits"].data_ptr(), L.stream())


def record_tail(L, out):
    B, T, D, MID = TAIL["B"], TAIL["T"], TAIL["D"], TAIL["MID"]
    for C in TAIL_C:
        P, h, w, (y, y_b, bad_y, bad_yb) = tail_inputs(C)
        P = [cuda(p) for p in P]
        h_d, len_d, w_d = cuda(h), cuda(torch.tensor(TAIL["lengths"], dtype=torch.int32)), cuda(w)
        y_d, ya_d, yb_d, ybw_d = cuda(y), cuda(bad_y), cuda(bad_yb), cuda(y_b)
        den_d = torch.full((1,), -7.0, device="cuda")
        L.call("ss_class_weight_sum", ya_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
        out[f"tail/C{C}/den"] = den_d.cpu().numpy()
        for drop in TAIL_DROP:
            for name, weighted, lam in VARIANTS:
                key = f"tail/C{C}/drop{drop[0]}/{name}"
                lam_d = None if lam is None else torch.tensor([lam], device="cuda")
                first, second = mix_labels(lam, y_d, ybw_d, ya_d, yb_d)

                def outs(n):
                    return dict(logits=torch.full((n, C), 5.0, device="cuda"), d_logits=torch.full((n, C), 3.0, device="cuda"),
                                loss=torch.zeros(1, device="cuda"), hits=torch.zeros(1, device="cuda", dtype=torch.int32))

                o = outs(B)
                tail_call(L, weighted, lam_d, P, h_d.data_ptr(), len_d.data_ptr(), first.data_ptr(), second.data_ptr(), B, C, drop,
                          DROP_OFFSET, float(B), w_d, den_d, o)
                rows = []
                for b in range(B):  # clip b as a launch of its own (its dropout counters start MID / 4 per clip further on)
                    ob = outs(1)
                    tail_call(L, weighted, lam_d, P, h_d.data_ptr() + 4 * b * T * D, len_d.data_ptr() + 4 * b,
                              first.data_ptr() + 8 * b, second.data_ptr() + 8 * b, 1, C, drop, DROP_OFFSET + b * MID // 4, float(B),
                              w_d, den_d, ob)
                    rows.append(ob)
                torch.cuda.synchronize()
                for b in range(B):  # a workgroup per clip: the launch of one clip writes that clip's rows of the batch launch
                    assert torch.equal(rows[b]["logits"][0], o["logits"][b]) and torch.equal(rows[b]["d_logits"][0], o["d_logits"][b])
                lkey = f"tail/C{C}/drop{drop[0]}/logits"  # (the logits do not depend on the loss: stored once)
                out.setdefault(lkey, o["logits"].cpu().numpy())
                assert np.array_equal(out[lkey], o["logits"].cpu().numpy()), key
                out[key + "/d_logits"] = o["d_logits"].cpu().numpy()
                out[key + "/hits"] = o["hits"].cpu().numpy()
                out[key + "/loss_rows"] = np.concatenate([r["loss"].cpu().numpy() for r in rows])
                out[key + "/loss_sum_any_order"] = o["loss"].cpu().numpy()


def record():
    """-> {name: array}: run every case on the current device through the C ABI."""
    from silent_speech_amd import _lib as L

    L.load()
    out = {}
    record_ce(L, out)
    record_tail(L, out)
    return out


def pack(out):
    """One float32 and one int32 array behind an index of (dtype, offset, shape) per name: 360 zip members cost more than their data."""
    flat, index = {"float32": [], "int32": []}, {}
    for k, v in out.items():
        dt = str(v.dtype)
        index[k] = [dt, int(sum(a.size for a in flat[dt])), list(v.shape)]
        flat[dt].append(v.reshape(-1))
    return index, {dt: np.concatenate(a) for dt, a in flat.items()}


def load(path):
    """-> (header, {name: array}) of a fixture ``main`` wrote."""
    z = np.load(path)
    header = json.loads(str(z["header"]))
    out = {k: z[dt][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape) for k, (dt, off, shape) in header["index"].items()}
    return header, out


def main(path):
    root = os.path.dirname(os.path.dirname(HERE))
    commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    header = {"what": "outputs of the nine loss entry points for the cases of tests/golden/make_loss_golden.py, one MI355X",
              "recorded_with": "python tests/golden/make_loss_golden.py tests/golden/loss_bits.npz",
              "tree": f"commit {commit or os.environ.get('SS_GOLDEN_COMMIT', '?')} + tests/golden/make_loss_golden.py"}
    out = record()
    header["index"], flat = pack(out)
    np.savez_compressed(path, header=np.array(json.dumps(header)), **flat)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes; {header['tree']}")


if __name__ == "__main__":
    main(sys.argv[1])
