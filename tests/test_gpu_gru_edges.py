"""GPU: the four GRU recurrence families (gru.hip, gru_split.h, gru_bf16.hip, gru_bf16_pers.h) at their slice, part, grid and
chunk edges, against tests/gru_ref.py, inside guard bands, and through identities that hold bit for bit.

Every buffer a kernel writes (out, the stash, d_g, their bf16 copies, every workspace) sits between two 4 KiB bands of a
sentinel; the region handed to the kernel is exactly what the library asks for.  ``out`` and the stash are prefilled with a NaN
pattern: the stash keeps it on frames past a clip's end -- every caller of store_rows4 on ``save`` stores under ``valid``
(gru.hip ``if (p.save && valid)``, gru_split.h the same, gru_bf16.hip inside ``if (valid)``, gru_bf16_pers.h
``if (p.save && st_valid)``) -- while ``out`` and ``d_g`` get exact zeros there (gru_split.h ``f32x4 o = {0.f, ..}; if (valid)
{..}`` then ``if (clip_ok)`` store; d_g: store_rows4 under ``clip_ok`` alone with the gradients initialised to zero).

Why the identities are exact.  A clip is one column of the MFMA's N dimension and nothing is reduced across clips:
  gru_bf16.hip, gru_step_fwd_kernel:  ``fb[ks][c] = b < B ? *(hb + (long)b * H + k0 + 8 * g) : 0`` with ``b = CG * cg + 16 * c + li``
      (lane column li = clip), ``acc[c][q] = mfma_bf16(fa[ks][q], fb[ks][c], acc[c][q])``, and the four k slices of the waves are
      summed in a fixed order for the lane's own clip: ``for (w = 0; w < 4; ++w) s += red[((w * CT + wv) * 3 + q) * 64 + lane]``.
  gru_step_bwd_kernel: the same shape, ``carry += red[((w * CT + wv) * 64 + lane) * 4]``; ``dhz`` is indexed by the clip.
  gru.hip / gru_split.h / gru_bf16_pers.h: ``clip = b0 + i`` (``li``), B operand read at panel row ``i``; the multi-CU partial
      sums are added in source order (``for (q = 0; q < NGP; ++q) s0 += xv[2 * q]``, ``for (q = 0; q < P; ++q) sm[0] += ..``).
Only the bias gradients cross clips (row_sum over the 16 lanes of a row, then float atomics): they stay at a tolerance.
So a clip's rows depend on its own gi, d_out and length alone, for a fixed number of parts -- whatever its position in the
batch (permutation), whoever its neighbours are (subset), however long the padding is (T against T + 3; in the reverse
direction the clip then starts at another parity of the exchange ring), and the two directions mirror each other when their
weights are equal (a step on zero state adds exact zeros to the bias: ``ar = br`` then ``mfma(w, 0, ar)``).
The one-CU and the multi-CU form sum the contraction in different segments (gru_split.h: "a clip's state differs in the last
bits between a batch of <= 128 and a larger one"): no identity between them, both are held to the float64 reference.
"""
import ctypes
import functools

import pytest
import torch

import gru_ref as GR
from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 4096                      # bytes of sentinel on either side of every buffer
BAND_F32 = 0x7FC0DEAD             # a quiet NaN with a payload, as int32
FILL_F32 = 0x7FC0BEEF             # another one: the prefill of out and the stash
BAND_BF16 = 0x7FC1                # bf16 NaN; two of them make the int32 band word
BAND_WS = 0x5A
CAP_CUS = 160                     # any non-zero CU cap keeps the recurrences on six parts
F32_TOL = dict(out=2e-5, save=2e-5, dg=(3e-5, 1e-4), gb=(2e-4, 1e-4))   # test_gru_fwd_bwd's bounds (atol, rtol)
BF16_TOL = dict(out=2e-3, save=5e-3, dgi=2e-2, dw=3e-2)                 # test_gru_bf16_fwd_bwd's bounds


@pytest.fixture
def cu_cap(L):
    """The CU cap Trainer(micro_batches > 1) sets while its micro-batches run: the recurrences keep six parts."""
    L.call("ss_roi_cnn_set_max_workgroups", CAP_CUS)
    try:
        yield CAP_CUS
    finally:
        L.call("ss_roi_cnn_set_max_workgroups", 0)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------ guard bands
class Guarded:
    """``nbytes`` of device memory for a kernel between two GUARD-byte bands.  kind: "f32" (NaN-pattern bands, region prefilled
    with another NaN pattern), "bf16" (NaN bands and prefill), "ws" (0x5A bands, region zeroed: the state a workspace starts in)."""

    def __init__(self, name, kind, numel):
        self.name, self.kind = name, kind
        es = {"f32": 4, "bf16": 2, "ws": 1}[kind]
        self.nbytes = numel * es
        pad = -self.nbytes % 4  # the tail band starts on a word
        self.raw = torch.empty(GUARD + self.nbytes + pad + GUARD, dtype=torch.uint8, device="cuda")
        self.word = {"f32": BAND_F32, "bf16": BAND_BF16 << 16 | BAND_BF16, "ws": int.from_bytes(bytes([BAND_WS] * 4), "little")}[kind]
        self.raw.view(torch.int32).fill_(self.word)
        body = self.raw[GUARD:GUARD + self.nbytes]
        if kind == "f32":
            self.t = body.view(torch.float32)
            self.t.view(torch.int32).fill_(FILL_F32)
        elif kind == "bf16":
            self.t = body.view(torch.int16)
        else:
            self.t = body
            self.t.zero_()
        self.tail0 = GUARD + self.nbytes + pad

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        head, tail = self.raw[:GUARD].view(torch.int32), self.raw[self.tail0:].view(torch.int32)
        assert bool((head == self.word).all()), f"{self.name}: the band in front of the buffer was written"
        assert bool((tail == self.word).all()), f"{self.name}: the band behind the buffer was written"


def check_all(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check()


def is_fill(t):
    return t.contiguous().view(torch.int32) == FILL_F32


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, H, B, T, lengths=None, short=False, seed=0, bf16=False):
        g = torch.Generator().manual_seed(1000 * H + 7 * B + T + seed)
        self.H, self.B, self.T = H, B, T
        if lengths is None:
            top = T - 1 if short else T          # short: max(len) < T
            lengths = torch.randint(1, top + 1, (B,), generator=g)
            lengths[0] = top                     # one clip of the full length ..
            if B > 1:
                lengths[B - 1] = 1               # .. and one of a single frame, in the tail slice
        self.lengths = torch.as_tensor(lengths, dtype=torch.int64)
        if bf16:
            self.gi = torch.randn(2, B, T, 3 * H, generator=g) * 0.7
            self.whh = [torch.randn(3 * H, H, generator=g) / H ** 0.5 for _ in range(2)]
            self.bhh = [torch.randn(3 * H, generator=g) * 0.1 for _ in range(2)]
        else:
            a = 1.5 / H ** 0.5
            self.gi = torch.randn(2, B, T, 3 * H, generator=g) * 0.8
            self.whh = [(torch.rand(3 * H, H, generator=g) * 2 - 1) * a for _ in range(2)]
            self.bhh = [(torch.rand(3 * H, generator=g) * 2 - 1) * a for _ in range(2)]
        self.d_out = torch.randn(B, T, 2 * H, generator=g)
        self.valid = torch.arange(T)[None] < self.lengths[:, None]

    def take(self, idx, T=None):
        """The clips ``idx`` (a permutation or a subset) as a case of their own, optionally padded to T frames with NaN."""
        c = Case.__new__(Case)
        c.H, c.B, c.T = self.H, len(idx), T or self.T
        c.lengths = self.lengths[idx]
        c.whh, c.bhh = self.whh, self.bhh
        c.gi = torch.full((2, c.B, c.T, 3 * c.H), float("nan"))
        c.gi[:, :, :self.T] = self.gi[:, idx]
        c.d_out = torch.full((c.B, c.T, 2 * c.H), float("nan"))
        c.d_out[:, :self.T] = self.d_out[idx]
        c.valid = torch.arange(c.T)[None] < c.lengths[:, None]
        return c


# ------------------------------------------------------------------------------------------------------------ f32 runner
def run_f32(L, c, use_ws, cap_set=False, full=True):
    """ss_gru_fwd (stash) and ss_gru_bwd; ``full`` adds the stash-less forward, ss_gru_fwd_drop and the BPTT without bias
    gradients.  Guard bands, the sync header and the reported workspace size are checked here.  -> CPU tensors."""
    H, B, T, N = c.H, c.B, c.T, c.B * c.T
    d = GR.f32_dispatch(B, T, H, cus(), cap_set=cap_set, workspace=use_ws)
    nb = L.gru_sync_bytes(B, T, H)
    assert nb == GR.f32_dispatch(B, T, H, cus()).sync_bytes, "ss_gru_sync_bytes against the restated layout"
    # a workspace is handed in even where the library asks for none (nb == 0): the one-CU kernels must run and leave it alone
    ws = Guarded("sync_ws", "ws", nb if nb else 4096) if use_ws else None
    wp = ws.ptr() if ws else None
    dev = lambda x: x.contiguous().cuda()
    gi, len_d, dout = dev(c.gi.reshape(2, N, 3 * H)), dev(c.lengths.to(torch.int32)), dev(c.d_out.reshape(N, 2 * H))
    w = [dev(x) for x in c.whh]
    b = [dev(x) for x in c.bhh]
    out, save, dg = Guarded("out", "f32", N * 2 * H), Guarded("save", "f32", 2 * N * 4 * H), Guarded("d_g", "f32", 2 * N * 4 * H)
    bufs = [x for x in (out, save, dg, ws) if x is not None]
    fwd_args = lambda o, s: (gi.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), len_d.data_ptr(), B, T, H,
                             o, s)
    launches = 0
    L.call("ss_gru_fwd", *fwd_args(out.ptr(), save.ptr()), wp, L.stream())
    check_all(bufs)
    launches += 1
    if full:
        out2 = Guarded("out (no stash)", "f32", N * 2 * H)
        L.call("ss_gru_fwd", *fwd_args(out2.ptr(), None), wp, L.stream())
        check_all(bufs + [out2])
        assert torch.equal(out2.t, out.t), "the inference form gives other bits"
        out3, od3 = Guarded("out (drop)", "f32", N * 2 * H), Guarded("out_drop", "f32", N * 2 * H)
        args = fwd_args(out3.ptr(), None) + (od3.ptr(), 0.2, 1234, 5 << 40, wp, L.stream())
        if d.parts == 0:
            with pytest.raises(RuntimeError):  # the one-CU form has no fused dropout: the caller runs ss_dropout
                L.call("ss_gru_fwd_drop", *args)
        else:
            L.call("ss_gru_fwd_drop", *args)
            od_ref = torch.empty(N * 2 * H, device="cuda")
            L.call("ss_dropout", out.ptr(), od_ref.data_ptr(), N * 2 * H, 0.2, 1234, 5 << 40, None, L.stream())
            check_all(bufs + [out3, od3])
            assert torch.equal(out3.t, out.t) and torch.equal(od3.t, od_ref)
        launches += 2
    gb = torch.full((4, 3 * H), 0.5, device="cuda")  # (ih_f, hh_f, ih_r, hh_r), accumulated into
    bwd_args = lambda g: (dout.data_ptr(), out.ptr(), save.ptr(), w[0].data_ptr(), w[1].data_ptr(), len_d.data_ptr(), B, T, H, g,
                          0.0, 0, 0)
    L.call("ss_gru_bwd", *bwd_args(dg.ptr()), gb[0].data_ptr(), gb[1].data_ptr(), gb[2].data_ptr(), gb[3].data_ptr(), wp, L.stream())
    check_all(bufs)
    launches += 1
    if full:
        dg2 = Guarded("d_g (no bias)", "f32", 2 * N * 4 * H)
        L.call("ss_gru_bwd", *bwd_args(dg2.ptr()), None, None, None, None, wp, L.stream())
        check_all(bufs + [dg2])
        assert torch.equal(dg2.t, dg.t), "the BPTT without bias gradients gives other bits"
        launches += 1
    if ws is not None:
        hdr = ws.t[:GR.SYNC_HDR_WORDS * 4].view(torch.int32).cpu()
        if d.parts:
            assert int(hdr[2]) == 0, "a bounded wait on a partner workgroup gave up"
            assert int(hdr[1]) == 0, "workgroups of a finished launch still counted"
            assert int(hdr[0]) == launches, "the generation advances by one per launch"
        else:
            assert nb == 0 and not bool(ws.t.any()), "the one-CU form touched the workspace"
    return dict(out=out.t.cpu().view(B, T, 2 * H), save=save.t.cpu().view(2, B, T, 4, H), dg=dg.t.cpu().view(2, B, T, 4, H),
                gb=gb.cpu(), parts=d.parts)


def errs(got, ref, rtol=0.0):
    """(largest |got - ref|, largest excess over rtol * |ref|) in float64."""
    e = (got.double() - ref.double()).abs()
    return float(e.max()), float((e - rtol * ref.double().abs()).max())


def check_stash_sentinel(res, valid):
    keep = is_fill(res["save"])                       # (2, B, T, 4, H)
    inv = ~valid[None, :, :, None, None].expand_as(keep)
    assert bool(keep[inv].all()), "stash rows past a clip's end were written"
    assert not bool(keep[~inv].any()), "stash rows of valid frames were left out"


def check_f32(name, res, ref, c):
    """Against the float64 reference at the bounds of test_gru_fwd_bwd.  -> the measured errors."""
    m = {}
    assert torch.isfinite(res["out"]).all() and torch.isfinite(res["dg"]).all() and torch.isfinite(res["gb"]).all(), name
    check_stash_sentinel(res, c.valid)
    v5 = c.valid[None, :, :, None, None].double()
    m["out"], _ = errs(res["out"], ref.out)
    m["save"], _ = errs(torch.where(v5.bool(), res["save"].double(), torch.zeros((), dtype=torch.float64)), ref.save)
    m["dg"], dg_x = errs(res["dg"], ref.d_g, F32_TOL["dg"][1])
    gb_ref = torch.stack([ref.g_bih[0], ref.g_bhh[0], ref.g_bih[1], ref.g_bhh[1]]) + 0.5
    m["gb"], gb_x = errs(res["gb"], gb_ref, F32_TOL["gb"][1])
    print(f"GRU-EDGE f32 {name} H={c.H} B={c.B} T={c.T} parts={res['parts']}: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    assert m["out"] <= F32_TOL["out"], (name, m)
    assert m["save"] <= F32_TOL["save"], (name, m)
    assert dg_x <= F32_TOL["dg"][0], (name, m)
    assert gb_x <= F32_TOL["gb"][0], (name, m)
    # rows past a clip's end: exact zeros in out and d_g
    assert float(res["out"][~c.valid].abs().max() if (~c.valid).any() else 0) == 0
    assert float(res["dg"][:, ~c.valid].abs().sum()) == 0
    return m


# ------------------------------------------------------------------------------------------------------------ f32 routes
def f32_edge_batch(H, edge):
    """The batch of a named edge on this device, from the restated dispatch."""
    n, T = cus(), 3
    multi = [B for B in range(1, 4000) if GR.f32_dispatch(B, T, H, n).parts]
    if edge == "last_multi":
        return max(multi)
    if edge == "first_one_cu":
        return max(multi) + 1
    if edge == "last_twelve":
        return max(B for B in multi if GR.f32_dispatch(B, T, H, n).parts == 12)
    if edge == "first_six":
        return max(B for B in multi if GR.f32_dispatch(B, T, H, n).parts == 12) + 1
    return int(edge)


# what the issue's table says of each edge on a 256-CU part
F32_LITERAL = {(192, "last_twelve"): 128, (192, "first_six"): 129, (192, "last_multi"): 320, (192, "first_one_cu"): 321,
               (64, "last_multi"): 960, (64, "first_one_cu"): 961}
# (H, edge, T, max(len) < T)
F32_TABLE = [(192, "1", 5, False), (192, "15", 4, False), (192, "16", 3, False), (192, "17", 5, True),
             (192, "64", 3, False), (192, "65", 4, False), (192, "last_twelve", 3, False), (192, "first_six", 4, True),
             (192, "last_multi", 3, False), (192, "first_one_cu", 2, False),
             (64, "1", 5, False), (64, "17", 4, True), (64, "last_multi", 3, False), (64, "first_one_cu", 2, False)]
_F32_RUNS = {}


def f32_table_run(L, H, edge, T, short):
    """One edge: the multi-CU form (workspace) and the one-CU form (None) on the same clips, each against the reference.  Kept for
    the session: the batches on the co-residency bound run once."""
    key = (H, edge)
    if key not in _F32_RUNS:
        B = f32_edge_batch(H, edge)
        if cus() == 256 and key in F32_LITERAL:
            assert B == F32_LITERAL[key]
        c = Case(H, B, T, short=short)
        assert int(c.lengths.max()) == (T - 1 if short else T) and (B == 1 or int(c.lengths.min()) == 1)
        ref = GR.reference(c.gi, c.whh, c.bhh, c.lengths, d_out=c.d_out)
        multi = run_f32(L, c, use_ws=True)
        one = run_f32(L, c, use_ws=False)
        _F32_RUNS[key] = (c, ref, multi, one)
    return _F32_RUNS[key]


@pytest.mark.parametrize("H,edge,T,short", F32_TABLE, ids=[f"H{h}-B{e}-T{t}" + ("-short" if s else "") for h, e, t, s in F32_TABLE])
def test_f32_dispatch_edges(L, H, edge, T, short):
    c, ref, multi, one = f32_table_run(L, H, edge, T, short)
    d = GR.f32_dispatch(c.B, T, H, cus())
    if cus() == 256 and (H, c.B) in GR.F32_EDGES_256:
        assert (d.parts, d.sized_parts, d.pairs, d.grid_pairs, d.workgroups, d.part_major) == GR.F32_EDGES_256[(H, c.B)]
    assert multi["parts"] == d.parts and one["parts"] == 0
    if edge == "first_one_cu":
        assert d.parts == 0 and d.sync_bytes == 0
    check_f32("multi_cu" if d.parts else "one_cu(ws given)", multi, ref, c)
    check_f32("one_cu", one, ref, c)
    # no identity between the two forms (other contraction segments): their distance, for the record
    print(f"GRU-EDGE f32 one-CU against {d.parts or 1} parts H={H} B={c.B}: out {errs(multi['out'], one['out'])[0]:.3e}, "
          f"d_g {errs(multi['dg'], one['dg'])[0]:.3e}")


@pytest.mark.parametrize("B,T,short", [(16, 4, True), (128, 3, False), (129, 3, False)])
def test_f32_cu_cap_route(L, cu_cap, B, T, short):
    """While a CU cap is set the slices keep six parts at B <= 128 -- in the workspace ss_gru_sync_bytes lays out for twelve.
    Which kernel ran shows in the bits: the capped rows equal the rows the same clips get inside a batch of 129, which runs on
    six parts whatever the cap says (the subset identity of the module docstring)."""
    H = 192
    c = Case(H, B, T, short=short, seed=5)
    d = GR.f32_dispatch(B, T, H, cus(), cap_set=True)
    if cus() == 256:
        assert d.parts == 6 and d.sized_parts == (12 if B <= 128 else 6)
    ref = GR.reference(c.gi, c.whh, c.bhh, c.lengths, d_out=c.d_out)
    res = run_f32(L, c, use_ws=True, cap_set=True)
    assert res["parts"] == d.parts
    check_f32("cu_cap", res, ref, c)
    if B == 16 and cus() == 256:
        big = Case(H, 129, T, seed=6)
        big.gi[:, :B], big.d_out[:B], big.lengths[:B] = c.gi, c.d_out, c.lengths
        big.whh, big.bhh = c.whh, c.bhh
        big.valid = torch.arange(T)[None] < big.lengths[:, None]
        rb = run_f32(L, big, use_ws=True, cap_set=True, full=False)
        assert rb["parts"] == 6
        assert torch.equal(rb["out"][:B], res["out"]) and torch.equal(rb["dg"][:, :B], res["dg"])
        assert torch.equal(rb["save"][:, :B].contiguous().view(torch.int32), res["save"].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ bf16 runner
def run_bf16(L, c, persistent, full=True):
    """ss_gru_bf16_fwd and ss_gru_bf16_bwd with every by-product, on the persistent form (sync area) or the step kernels."""
    H, B, T, N = c.H, c.B, c.T, c.B * c.T
    lib = L.load()
    dev = lambda x: x.contiguous().cuda()
    wb = torch.empty(2, 3 * H, H, device="cuda", dtype=torch.int16)
    wtb = torch.empty(2, H, 3 * H, device="cuda", dtype=torch.int16)
    w_f, w_r = dev(c.whh[0]), dev(c.whh[1])
    L.call("ss_gru_bf16_prep", w_f.data_ptr(), w_r.data_ptr(), H, wb.data_ptr(), wtb.data_ptr(), None, None, 0, None, L.stream())
    nb = ctypes.c_long(0)
    assert lib.ss_gru_bf16_ws_bytes(B, H, ctypes.byref(nb)) == 0
    ws = Guarded("ws", "ws", nb.value)
    d = GR.bf16_dispatch(B, T, H, cus())
    assert lib.ss_gru_bf16_sync_bytes(B, T, H, ctypes.byref(nb)) == 0
    assert nb.value == d.sync_bytes, "ss_gru_bf16_sync_bytes against the restated layout"
    sync = Guarded("sync_ws", "ws", nb.value) if persistent else None
    sp, sn = (sync.ptr(), sync.nbytes) if sync else (None, 0)
    gi, lens, dout = dev(c.gi.reshape(2, N, 3 * H)), dev(c.lengths.to(torch.int32)), dev(c.d_out.reshape(N, 2 * H))
    b_f, b_r = dev(c.bhh[0]), dev(c.bhh[1])
    out, save = Guarded("out", "f32", N * 2 * H), Guarded("save", "f32", 2 * N * 4 * H)
    out_bf, out_drop_bf = Guarded("out_bf16", "bf16", N * 2 * H), Guarded("out_drop_bf16", "bf16", N * 2 * H)
    dg, dg_bf = Guarded("d_g", "f32", 2 * N * 4 * H), Guarded("d_g_bf16", "bf16", 2 * N * 4 * H)
    bufs = [x for x in (ws, sync, out, save, out_bf, out_drop_bf, dg, dg_bf) if x is not None]
    L.call("ss_gru_bf16_fwd", gi.data_ptr(), wb.data_ptr(), b_f.data_ptr(), b_r.data_ptr(), lens.data_ptr(), B, T, H, out.ptr(),
           save.ptr(), out_bf.ptr(), out_drop_bf.ptr(), 0.0, 0, 0, ws.ptr(), sp, sn, L.stream())
    check_all(bufs)
    calls = 1
    rb = lambda t: GR.bf(t.cpu())
    assert torch.equal(out_bf.t.cpu().view(torch.bfloat16).float(), rb(out.t)), "out_bf16 is not the rounding of out"
    assert torch.equal(out_drop_bf.t.cpu().view(torch.bfloat16).float(), rb(out.t)), "out_drop_bf16 at p = 0 is not the rounding of out"
    gb = [torch.full((3 * H,), 0.25, device="cuda") for _ in range(4)]  # d b_ih fwd, d b_hh fwd, d b_ih rev, d b_hh rev: added to
    L.call("ss_gru_bf16_bwd", dout.data_ptr(), out.ptr(), save.ptr(), wtb.data_ptr(), lens.data_ptr(), B, T, H, dg.ptr(), dg_bf.ptr(),
           0.0, 0, 0, *[t_.data_ptr() for t_ in gb], ws.ptr(), sp, sn, L.stream())
    check_all(bufs)
    calls += 1
    assert torch.equal(dg_bf.t.cpu().view(torch.bfloat16).float(), rb(dg.t)), "d_g_bf16 is not the rounding of d_g"
    if sync is not None and full:  # the f32 gate gradients are optional on the persistent form
        dg_bf2 = Guarded("d_g_bf16 alone", "bf16", 2 * N * 4 * H)
        L.call("ss_gru_bf16_bwd", dout.data_ptr(), out.ptr(), save.ptr(), wtb.data_ptr(), lens.data_ptr(), B, T, H, None, dg_bf2.ptr(),
               0.0, 0, 0, None, None, None, None, ws.ptr(), sp, sn, L.stream())
        check_all(bufs + [dg_bf2])
        calls += 1
        assert torch.equal(dg_bf2.t, dg_bf.t)
    if sync is not None:
        hdr = sync.t[:GR.SYNC_HDR_WORDS * 4].view(torch.int32).cpu()
        assert int(hdr[2]) == 0, "a bounded wait of the persistent recurrence gave up"
        assert int(hdr[1]) == 0
        assert int(hdr[0]) == calls * len(d.launches), "the generation advances by one per clip chunk and call"
    return dict(out=out.t.cpu().view(B, T, 2 * H), save=save.t.cpu().view(2, B, T, 4, H), dg=dg.t.cpu().view(2, B, T, 4, H),
                gb=torch.stack(gb).cpu(), chunks=d.launches)


def check_bf16(name, res, ref, c):
    """Against the bf16-emulating reference at the bounds of test_gru_bf16_fwd_bwd.  -> the measured errors."""
    H, B, T = c.H, c.B, c.T
    m = {}
    assert torch.isfinite(res["out"]).all() and torch.isfinite(res["dg"]).all() and torch.isfinite(res["gb"]).all(), name
    check_stash_sentinel(res, c.valid)
    v5 = c.valid[None, :, :, None, None]
    m["out"] = errs(res["out"], ref.out)[0]
    m["save"] = errs(torch.where(v5, res["save"], torch.zeros(())), ref.save)[0]
    for d in range(2):
        scale = float(ref.d_g[d, :, :, :3].abs().max())
        m[f"dgi{d}"] = errs(res["dg"][d, :, :, :3], ref.d_g[d, :, :, :3])[0] / scale
        dgh = torch.cat([res["dg"][d, :, :, 0], res["dg"][d, :, :, 1], res["dg"][d, :, :, 3]], 2)
        h = ref.out[:, :, d * H:(d + 1) * H]
        hprev = torch.zeros_like(h)
        if d == 0:
            hprev[:, 1:] = h[:, :-1]
        else:
            hprev[:, :-1] = h[:, 1:]
        dW = torch.einsum("btg,bth->gh", dgh, hprev)
        m[f"dw{d}"] = errs(dW, ref.g_whh[d])[0] / (float(ref.g_whh[d].abs().max()) or scale)
    # the bias gradients: the column sums of the kernel's own d_g over ALL clips (a chunk that overwrote instead of adding would
    # leave the last chunk's sums), at the existing bound; and the reference's sums, relative to their largest like d gi
    cs = res["dg"].double().sum((1, 2))  # (2, 4, H)
    gb_ref = torch.stack([ref.g_bih[0], ref.g_bhh[0], ref.g_bih[1], ref.g_bhh[1]])
    for d in range(2):
        for got, want in ((res["gb"][2 * d], cs[d, :3].reshape(-1)), (res["gb"][2 * d + 1], torch.cat([cs[d, 0], cs[d, 1], cs[d, 3]]))):
            assert errs(got - 0.25, want)[0] < 1e-4 * max(1.0, float(want.abs().max())), (name, d)
    m["gb"] = errs(res["gb"] - 0.25, gb_ref)[0] / float(gb_ref.abs().max())
    print(f"GRU-EDGE bf16 {name} H={H} B={B} T={T} chunks={res['chunks']}: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    assert m["out"] < BF16_TOL["out"] and m["save"] < BF16_TOL["save"], (name, m)
    for d in range(2):
        assert m[f"dgi{d}"] < BF16_TOL["dgi"] and m[f"dw{d}"] < BF16_TOL["dw"], (name, m)
    assert m["gb"] < BF16_TOL["dgi"], (name, m)
    assert float(res["out"][~c.valid].abs().max() if (~c.valid).any() else 0) == 0
    assert float(res["dg"][:, ~c.valid].abs().sum()) == 0
    return m


def bf16_edge_batch(H, edge):
    n = cus()
    single = [B for B in range(1, 3000) if len(GR.bf16_dispatch(B, 2, H, n).launches) == 1]
    if edge == "last_single":
        return max(single)
    if edge == "first_split":
        return max(single) + 1
    if edge == "no_round_up":  # the first batch whose equal chunks cannot be rounded up to 4 slices
        P = H // GR.PUNITS
        slices = n // (2 * P)
        for B in range(max(single) + 1, 6000, 16):
            need = GR.ceil_div(B, 16)
            per = GR.ceil_div(need, GR.ceil_div(need, slices))
            if GR.ceil_div(per, 4) * 4 > slices:
                return B
    return int(edge)


BF16_LITERAL = {(128, "last_single"): 1024, (128, "first_split"): 1025, (256, "last_single"): 512, (256, "first_split"): 513,
                (384, "last_single"): 336, (384, "first_split"): 337, (512, "last_single"): 256, (512, "first_split"): 257,
                (384, "no_round_up"): 641}
# (H, edge, T, max(len) < T)
BF16_TABLE = [(128, "1", 3, False), (128, "17", 3, True), (128, "last_single", 2, False), (128, "first_split", 2, False),
              (256, "last_single", 2, False), (256, "first_split", 3, False), (384, "last_single", 2, False),
              (384, "first_split", 3, True), (384, "no_round_up", 2, False), (512, "last_single", 2, False),
              (512, "first_split", 3, False)]


@functools.lru_cache(maxsize=None)
def bf16_table_case(H, edge, T, short):
    B = bf16_edge_batch(H, edge)
    if cus() == 256 and (H, edge) in BF16_LITERAL:
        assert B == BF16_LITERAL[(H, edge)]
    c = Case(H, B, T, short=short, bf16=True)
    return c, GR.reference(c.gi, c.whh, c.bhh, c.lengths, d_out=c.d_out, bf16=True)


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("H,edge,T,short", BF16_TABLE, ids=[f"H{h}-B{e}-T{t}" + ("-short" if s else "") for h, e, t, s in BF16_TABLE])
def test_bf16_chunk_edges(L, H, edge, T, short, persistent):
    c, ref = bf16_table_case(H, edge, T, short)
    d = GR.bf16_dispatch(c.B, T, H, cus())
    if cus() == 256 and (H, c.B) in GR.BF16_EDGES_256:
        assert d.launches == GR.BF16_EDGES_256[(H, c.B)]
    if edge == "last_single":
        assert len(d.launches) == 1
    if edge in ("first_split", "no_round_up"):
        assert len(d.launches) == 2
    res = run_bf16(L, c, persistent)
    assert res["chunks"] == d.launches
    check_bf16("persistent" if persistent else "step", res, ref, c)


# ------------------------------------------------------------------------------------------------------------ identities
# name -> (family, H, workspace / persistent, CU cap set, parts at 256 CUs for the identity batches)
ROUTES = {"f32_one_cu": ("f32", 192, False, False, 0), "f32_twelve": ("f32", 192, True, False, 12), "f32_six": ("f32", 192, True, True, 6),
          "f32_two": ("f32", 64, True, False, 2), "bf16_persistent": ("bf16", 256, True, False, None),
          "bf16_step": ("bf16", 256, False, False, None)}


class Route:
    def __init__(self, L, name):
        self.L, self.name = L, name
        self.family, self.H, self.ws, self.cap, self.parts = ROUTES[name]
        self.B = 37 if self.family == "f32" else 70

    def case(self, T, lengths=None, short=False):
        return Case(self.H, self.B, T, lengths=lengths, short=short, bf16=self.family == "bf16", seed=11)

    def run(self, c):
        if self.family == "f32":
            res = run_f32(self.L, c, use_ws=self.ws, cap_set=self.cap, full=False)
            if cus() == 256:
                assert res["parts"] == self.parts
        else:
            res = run_bf16(self.L, c, self.ws, full=False)
        check_stash_sentinel(res, c.valid)
        assert torch.isfinite(res["out"]).all() and torch.isfinite(res["dg"]).all()
        return res


@pytest.fixture(params=sorted(ROUTES))
def route(L, request):
    r = Route(L, request.param)
    if r.cap:
        L.call("ss_roi_cnn_set_max_workgroups", CAP_CUS)
    try:
        yield r
    finally:
        L.call("ss_roi_cnn_set_max_workgroups", 0)


def same_rows(a, b, what):
    """out, stash and d_g bit for bit (the stash through its bits: its untouched rows hold a NaN pattern)."""
    assert torch.equal(a["out"], b["out"]), what + ": out"
    assert torch.equal(a["dg"], b["dg"]), what + ": d_g"
    assert torch.equal(a["save"].contiguous().view(torch.int32), b["save"].contiguous().view(torch.int32)), what + ": stash"


def rows(res, idx, T=None):
    """The rows of the clips ``idx`` (and of the first T frames) of a run."""
    return dict(out=res["out"][idx][:, :T], save=res["save"][:, idx][:, :, :T], dg=res["dg"][:, idx][:, :, :T])


def test_identity_permutation(route):
    """The same clips in another order give the permuted rows: 11 b + 20 mod B moves clips between all slices, the partial tail
    slice included."""
    B = route.B
    perm = (11 * torch.arange(B) + 20) % B
    assert sorted(perm.tolist()) == list(range(B))
    src, dst, tail = perm // 16, torch.arange(B) // 16, (B - 1) // 16
    assert B % 16 and bool((src[dst == tail] != tail).any()) and bool((dst[src == tail] != tail).any())  # into and out of the tail
    assert bool((src[dst == 0] != 0).any())
    c = route.case(T=5)
    a, b = route.run(c), route.run(c.take(perm))
    same_rows(rows(a, perm), b, "permuted batch")


def test_identity_padding(route):
    """T against T + 3 with NaN in the extra frames of gi and d_out: equal rows for t < T, exact zeros behind (the reverse
    direction starts three steps later: the other parity of the exchange ring)."""
    c = route.case(T=4)
    idx = torch.arange(c.B)
    a, b = route.run(c), route.run(c.take(idx, T=7))
    same_rows(a, rows(b, idx, T=4), "padded batch")
    assert float(b["out"][:, 4:].abs().max()) == 0 and float(b["dg"][:, :, 4:].abs().max()) == 0


def test_identity_mirror(route):
    """Reverse weights = forward weights and reverse inputs = each clip's forward inputs in reverse order: the reverse
    direction's rows are the forward direction's, mirrored inside each clip.  Ragged, max(len) < T."""
    H, T = route.H, 5
    c = route.case(T=T, short=True)
    B = c.B
    c.whh, c.bhh = [c.whh[0], c.whh[0].clone()], [c.bhh[0], c.bhh[0].clone()]
    mir = (c.lengths[:, None] - 1 - torch.arange(T)[None]).clamp(min=0)      # (B, T): len - 1 - t on valid frames
    take = lambda x: x.gather(1, mir[:, :, None].expand(B, T, x.shape[2]))
    nan = float("nan")
    c.gi[1] = torch.where(c.valid[:, :, None], take(c.gi[0]), torch.full((), nan))
    c.d_out[:, :, H:] = torch.where(c.valid[:, :, None], take(c.d_out[:, :, :H]), torch.full((), nan))
    r = route.run(c)
    v = c.valid[:, :, None]
    z = torch.zeros(())
    assert torch.equal(torch.where(v, r["out"][:, :, H:], z), torch.where(v, take(r["out"][:, :, :H]), z)), "out"
    for k in ("dg", "save"):
        fwd, rev = r[k][0].reshape(B, T, 4 * H), r[k][1].reshape(B, T, 4 * H)
        assert torch.equal(torch.where(v, rev, z), torch.where(v, take(fwd), z)), k


# (route, H, B, b, parts at 256 CUs): the first b clips of a batch of B against a run on those alone, same parts in both
SUBSETS = [("f32", 192, 128, 5, 12), ("f32", 192, 320, 129, 6), ("f32", 64, 250, 3, 2), ("bf16", 512, 257, 65, None)]


@pytest.mark.parametrize("form", ["multi", "single"])
@pytest.mark.parametrize("family,H,B,b,parts", SUBSETS, ids=[f"{f}-H{h}-{B}-{b}" for f, h, B, b, _ in SUBSETS])
def test_identity_subset(L, family, H, B, b, parts, form):
    """``multi`` = the multi-CU resp. persistent form, ``single`` = one CU per slice resp. the step kernels."""
    T = 3
    idx = torch.arange(b)
    if family == "f32":
        if form == "multi":
            n = cus()
            if GR.f32_dispatch(B, T, H, n).parts != GR.f32_dispatch(b, T, H, n).parts:
                pytest.fail(f"{B} and {b} clips run on different parts on {n} CUs: choose the pair from the restatement")
            if n == 256:
                assert GR.f32_dispatch(B, T, H, n).parts == parts
        if (H, B) == (192, 320) and form == "multi" and cus() == 256:  # the batch on the bound runs once a session
            c, _, big, _ = f32_table_run(L, 192, "last_multi", 3, False)
        elif (H, B) == (192, 320) and form == "single" and cus() == 256:
            c, _, _, big = f32_table_run(L, 192, "last_multi", 3, False)
        else:
            c = Case(H, B, T, seed=3)
            big = run_f32(L, c, use_ws=form == "multi", full=False)
        small = run_f32(L, c.take(idx), use_ws=form == "multi", full=False)
    else:
        c = Case(H, B, T, seed=3, bf16=True)
        big = run_bf16(L, c, form == "multi", full=False)
        small = run_bf16(L, c.take(idx), form == "multi", full=False)
    same_rows(rows(big, idx), small, f"first {b} of {B}")
