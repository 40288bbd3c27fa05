"""GPU: the host-side launch state of csrc/launch.h -- the dynamic-LDS limit raised once per (device, kernel), the CU count kept
per device, the workgroup cap behind every persistent grid.

The bounds are the run-to-run bounds the other suites already hold identical launches to:
  logits            bit-equal (test_gpu_model.py / test_gpu_model_c5.py: a repeated forward is ``torch.equal``)
  f32 step          loss to 1e-6 relative, gradients to 1e-5 of the largest entry (test_gpu_model.py, the bench's dumped step)
  config-5 step     loss to 1e-5, gradient norm to 1e-3 relative (test_gpu_model_c5.py::test_c5_micro_batches), gradients to 1e-5
                    of the largest entry like the f32 step's
  wide-tile GEMM    2e-5 sqrt(K) + 1e-5 |ref| against float64 (test_gpu_kernels.py::test_gemm_input_projection_wide_tiles),
                    and the plain stores of two launches bit-equal
  f32 ROI CNN       forward bit-equal whichever workgroup computes a frame, gradients to 2e-5 of the largest entry
                    (test_gpu_kernels.py::test_roi_cnn_stash_and_bwd)
  config-5 CNN      bf16 maps as ``assert_bf16_close``, features to 2e-5, embeddings to 5e-5 (test_gpu_bf16.py)"""
import os
import subprocess
import sys

import pytest
import torch

from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(mode, tmp_path):
    out = str(tmp_path / (mode + ".pt"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_launch_state_child.py"), mode, out], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a launcher's status other than 0 raises in the child)
    return torch.load(out, map_location="cpu", weights_only=False)


def check_same_step(name, a, b):
    scale = float(a["grads"].abs().max())
    d_grad = float((a["grads"] - b["grads"]).abs().max())
    d_logit = float((a["logits"] - b["logits"]).abs().max())
    print(f"{name}: loss {a['loss']:.8f} / {b['loss']:.8f}, gradient norm {a['grad_norm']:.6e} / {b['grad_norm']:.6e}, "
          f"logits differ by {d_logit:.2e}, gradients by {d_grad:.2e} (largest entry {scale:.2e})")
    assert torch.isfinite(a["logits"]).all() and torch.isfinite(a["grads"]).all() and scale > 0
    assert torch.equal(a["logits"], b["logits"]), (name, d_logit)
    assert d_grad <= 1e-5 * scale, (name, d_grad, scale)
    if name == "f32":
        assert abs(a["loss"] - b["loss"]) <= 1e-6 * abs(a["loss"]), name
    else:
        assert abs(a["loss"] - b["loss"]) < 1e-5, name
        assert abs(a["grad_norm"] - b["grad_norm"]) < 1e-3 * a["grad_norm"], name


def check_same_gemm(a, b):
    K = 116
    for which, r in (("first", a), ("second", b)):
        err = (r["rows"].double() - r["ref"].double()).abs()
        print(f"wide-tile GEMM, {which}: max error {float(err.max()):.2e} against float64")
        assert bool((err <= 2e-5 * K ** 0.5 + 1e-5 * r["ref"].double().abs()).all()), (which, float(err.max()))
    assert torch.equal(a["rows"], b["rows"])


def check_all(got):
    check_same_gemm(*got.pop("wide_gemm"))
    assert sorted(got) == ["c5", "f32"]
    for name, (a, b) in got.items():
        check_same_step(name, a, b)


def test_attribute_is_set_once_and_the_second_launch_matches_the_first(L, tmp_path):
    """In a fresh process the first f32 step, the first config-5 step and the first wide-tile GEMM raise the LDS limit of every
    kernel they launch; the second of each, from the same state, finds it raised and must compute the same."""
    check_all(run_child("twice", tmp_path))


def test_a_second_device_gets_its_own_state(L, tmp_path):
    """The same steps and GEMM on device 0, then on device 1 of one process: every launcher returns 0 there (its kernels' limits are
    raised on that device too, its grids are sized by that device) and the two devices agree."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"needs two devices in one process; torch.cuda.device_count() is {n} here")
    check_all(run_child("two_devices", tmp_path))


def _bf16_close(name, got, ref):  # test_gpu_bf16.py::assert_bf16_close
    refb = ref.to(torch.bfloat16).to(torch.float32)
    err = (got - ref).abs()
    tol = 2.0 ** -7 * ref.abs() + 1e-6 * max(1.0, float(ref.abs().max()))
    assert bool((err <= tol).all()), f"{name}: max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})"
    assert (got == refb).float().mean().item() >= 0.995, name


def test_workgroup_cap_still_shapes_every_persistent_grid(L):
    """ss_roi_cnn_set_max_workgroups(3) with 7 frames: the persistent CNN kernels compute what they compute without the cap.  (With
    the cap in effect a workgroup walks two or three frames instead of one; the grid itself is not observable through the C ABI, so
    that the cap took effect is not shown here -- a grid that ignored it would pass too.)"""
    import weights as W

    N, E = 7, 32
    g = torch.Generator().manual_seed(5)
    keys = ("roi_cnn.net.0.weight", "roi_cnn.net.0.bias", "roi_cnn.net.3.weight", "roi_cnn.net.3.bias", "roi_cnn.net.6.weight",
            "roi_cnn.net.6.bias", "roi_cnn.fc.weight", "roi_cnn.fc.bias")
    sd = W.make_state_dict(5, 84, 5, True)
    P = [sd[k].cuda() for k in keys]
    R32 = torch.randint(0, 256, (N, 32, 32), generator=g, dtype=torch.uint8).cuda()
    d_out = torch.randn(N, E, generator=g).cuda()
    sizes = L.cnn_stash_sizes(32, 32)
    n_a1, n_a2, n_i1, n_i2, n_m3, n_feat = sizes
    # config 5: frame -> conv1 + conv2 -> conv3 -> conv_last + Linear
    R96 = torch.randint(0, 256, (N, 96, 96), generator=g, dtype=torch.uint8).cuda()
    C = (1, 16, 32, 64, 96)
    w = [(torch.randn(C[i + 1], C[i], 3, 3, generator=g) / (3.0 * C[i] ** 0.5)).cuda() for i in range(4)]
    b = [(torch.randn(C[i + 1], generator=g) * 0.1).cuda() for i in range(4)]
    wfc, bfc = (torch.randn(64, 96, generator=g) / 10.0).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()

    def run(cap):
        L.call("ss_roi_cnn_set_max_workgroups", cap)
        try:
            out = torch.zeros(N, E, device="cuda")
            st = [torch.zeros(N, n_a1, device="cuda"), torch.zeros(N, n_i1, device="cuda", dtype=torch.uint8),
                  torch.zeros(N, n_a2, device="cuda"), torch.zeros(N, n_i2, device="cuda", dtype=torch.uint8),
                  torch.zeros(N, n_m3, device="cuda", dtype=torch.uint8), torch.zeros(N, n_feat, device="cuda")]
            G = [torch.zeros_like(p) for p in P]
            L.call("ss_roi_cnn_fwd_stash", R32.data_ptr(), N, 32, 32, 1, *[p.data_ptr() for p in P], E, out.data_ptr(), E,
                   *[s.data_ptr() for s in st], sizes.ptr, L.stream())
            L.call("ss_roi_cnn_bwd", R32.data_ptr(), N, 32, 32, 1, *[p.data_ptr() for p in P], E, *[s.data_ptr() for s in st],
                   sizes.ptr, d_out.data_ptr(), E, *[gg.data_ptr() for gg in G], L.stream())
            a2 = torch.zeros(N, 24, 24, 32, device="cuda", dtype=torch.int16)
            i2 = torch.zeros(N, 24, 24, 32, device="cuda", dtype=torch.uint8)
            a3 = torch.zeros(N, 12, 12, 64, device="cuda", dtype=torch.int16)
            i3 = torch.zeros(N, 12, 12, 64, device="cuda", dtype=torch.uint8)
            stat = torch.zeros(N, 2, device="cuda")
            z = torch.zeros(N, 64, device="cuda")
            mask = torch.zeros(N, 144, 96, device="cuda", dtype=torch.uint8)
            feat = torch.zeros(N, 96, device="cuda")
            L.call("ss_c5_conv12_fwd", R96.data_ptr(), N, 1, w[0].data_ptr(), b[0].data_ptr(), w[1].data_ptr(), b[1].data_ptr(),
                   a2.data_ptr(), i2.data_ptr(), stat.data_ptr(), L.stream())
            L.call("ss_c5_conv_fwd", 3, a2.data_ptr(), N, w[2].data_ptr(), b[2].data_ptr(), a3.data_ptr(), i3.data_ptr(), L.stream())
            L.call("ss_c5_conv_last_fwd", a3.data_ptr(), N, w[3].data_ptr(), b[3].data_ptr(), wfc.data_ptr(), bfc.data_ptr(), 64,
                   z.data_ptr(), 64, mask.data_ptr(), feat.data_ptr(), L.stream())
            torch.cuda.synchronize()
        finally:
            L.call("ss_roi_cnn_set_max_workgroups", 0)
        bf = lambda t: t.cpu().view(torch.bfloat16).float()  # noqa: E731
        return dict(out=out.cpu(), G=[gg.cpu() for gg in G], a2=bf(a2), i2=i2.cpu(), a3=bf(a3), i3=i3.cpu(), stat=stat.cpu(),
                    feat=feat.cpu(), z=z.cpu(), mask=mask.cpu())

    free, capped = run(0), run(3)
    assert float(free["out"].abs().max()) > 0 and float(free["z"].abs().max()) > 0 and float(free["a3"].abs().max()) > 0
    assert torch.equal(capped["out"], free["out"]), "the forward output of a frame must not depend on which workgroup computes it"
    for k, a, ref in zip(keys, capped["G"], free["G"]):
        scale = max(float(ref.abs().max()), 1e-6)
        diff = float((a - ref).abs().max())
        print(f"f32 ROI CNN, cap 3 against no cap, d {k}: {diff:.2e} of {scale:.2e}")
        assert scale > 1e-6 and diff < 2e-5 * scale, (k, diff, scale)
    assert torch.equal(capped["stat"], free["stat"])
    _bf16_close("a2", capped["a2"], free["a2"])
    _bf16_close("a3", capped["a3"], free["a3"])
    d_feat, d_z = float((capped["feat"] - free["feat"]).abs().max()), float((capped["z"] - free["z"]).abs().max())
    print(f"config-5 chain, cap 3 against no cap: features differ by {d_feat:.2e}, embeddings by {d_z:.2e}, "
          f"{int((capped['i2'] != free['i2']).sum())} + {int((capped['i3'] != free['i3']).sum())} pool winners, "
          f"{int((capped['mask'] != free['mask']).sum())} mask bytes")
    assert d_feat < 2e-5 and d_z < 5e-5
    assert torch.equal(capped["i2"], free["i2"]) and torch.equal(capped["i3"], free["i3"]) and torch.equal(capped["mask"], free["mask"])
