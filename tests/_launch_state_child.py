"""Child process of tests/test_gpu_launch_state.py: a fresh process, so that the first launch of every kernel that asks for more
than 64 KB of dynamic LDS is the one that raises its limit (csrc/launch.h) and the second one finds the limit raised.

    python _launch_state_child.py twice OUT         one f32 and one bf16 config-5 training step and one wide-tile GEMM, each
                                                    twice, on device 0
    python _launch_state_child.py two_devices OUT   each of the three once on device 0, then once on device 1

Every step starts from the same seeded state.  A kernel that returns a status other than 0 raises in ``_lib.call``; the logits,
gradients, loss and gradient norm of every step, and rows of the GEMM's output, go to OUT for the parent to compare."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

# f32: the fused 64x64 ROI kernels (80 / 160 KB of LDS) and the grouped weight-gradient GEMM.  bf16: B T and B (T - 1) are
# multiples of 64 (the grouped ring kernel), roi_emb = 64 (d layer_in through the ring kernel), every config-5 CNN kernel.
# gemm_wide_kc_kernel needs 80 % of the chip in 192 x 192 tiles, which no small training step has: wide_gemm() calls it directly
CASES = {
    "f32": dict(seed=31, B=2, T=4, classes=5, roi=(64, 64), model=dict(hidden=192)),
    "c5": dict(seed=32, B=64, T=3, classes=100, roi=(96, 96),
               model=dict(roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96), precision="bf16")),
}


def one_step(name: str, device: int) -> dict:
    import torch
    import weights as W
    import silent_speech_amd as ss

    c = CASES[name]
    shape = {k: v for k, v in c["model"].items() if k != "precision"}
    sd = W.make_state_dict(c["seed"], 84, c["classes"], True, **shape)
    X, Lh, R, y = W.make_inputs(c["seed"], c["B"], c["T"], 84, c["classes"], c["roi"])
    with torch.cuda.device(device):
        m = ss.BiGRUClassifier(84, c["classes"], use_roi=True, **c["model"])
        m.load_state_dict(sd)
        m.cuda().train()
        tr = ss.Trainer(m, dropout=False)
        Xd, Rd = X.cuda(), R.cuda()
        loss, _ = tr.step(Xd, Lh.cuda(), Rd, y.cuda())
        torch.cuda.synchronize()
        logits = m._workspace(Xd, Rd, train=True, slot=0).logits
        assert m.flat_grads.device.index == device and logits.device.index == device
        return dict(loss=float(loss), grad_norm=float(tr.grad_norm()), logits=logits.cpu().clone(), grads=m.flat_grads.cpu().clone())


WIDE = dict(M=7680, N=576, K=116, batch=2)  # config 2's layer-0 input projection: 240 tiles (test_gpu_kernels.py)


def wide_gemm(device: int) -> dict:
    """C = A B^T + bias on the wide-tile kernel; every 64th row of C (each row of tiles three times) and its float64 reference."""
    import torch
    from silent_speech_amd import _lib as L

    L.load()
    M, N, K, batch = WIDE["M"], WIDE["N"], WIDE["K"], WIDE["batch"]
    g = torch.Generator().manual_seed(M + N + K)
    A, Bm, bias = torch.randn(M, K, generator=g), torch.randn(batch, N, K, generator=g), torch.randn(batch, N, generator=g)
    with torch.cuda.device(device):
        a_d, b_d, bias_d = A.cuda(), Bm.cuda(), bias.cuda()
        c_d = torch.full((batch, M, N), 7.0, device="cuda")
        L.call("ss_gemm_f32_batched", 1, 1, M, N, K, a_d.data_ptr(), K, 2**31 - 1, 0, 0, b_d.data_ptr(), K, 2**31 - 1, 0, 0,
               c_d.data_ptr(), N, bias_d.data_ptr(), None, 0, 1, batch, 0, N * K, M * N, N, 0, L.stream())
        torch.cuda.synchronize()
        rows = c_d[:, ::64].cpu().clone()
    ref = (torch.einsum("mk,bnk->bmn", A[::64].double(), Bm.double()) + bias.double()[:, None, :]).float()
    return dict(rows=rows, ref=ref)


def main(mode: str, out_path: str) -> None:
    import torch

    devices = (0, 0) if mode == "twice" else (0, 1)
    got = {name: [one_step(name, d) for d in devices] for name in CASES}
    got["wide_gemm"] = [wide_gemm(d) for d in devices]
    torch.save(got, out_path)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
