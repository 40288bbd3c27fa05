"""The host references of tests/gru_ref.py, pinned without a GPU: the float64 recurrence against torch.nn.GRU on packed ragged
batches, and the restated dispatch against the edges the comments of gru_split.h / gru_bf16_pers.h give for a 256-CU part."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import gru_ref as GR


# ------------------------------------------------------------------------------------------------------------ the recurrence
@pytest.mark.parametrize("B,T,H,lengths", [(5, 7, 8, [7, 1, 4, 2, 6]), (3, 4, 16, [2, 3, 1]), (1, 3, 8, [3]), (9, 6, 12, None)])
def test_reference_matches_packed_nn_gru(B, T, H, lengths):
    """out, d gi and the bias gradients of the float64 reference against nn.GRU(bidirectional) over pack_padded_sequence, the
    input projection taken out of it: gi = W_ih x + b_ih with W_ih = identity blocks is not available in nn.GRU, so the module
    gets x and the reference gets the module's own W_ih x + b_ih."""
    g = torch.Generator().manual_seed(B * 100 + T * 10 + H)
    In = 5
    if lengths is None:
        lengths = torch.randint(1, T, (B,), generator=g).tolist()  # max(len) < T
    lengths = torch.tensor(lengths)
    gru = torch.nn.GRU(In, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    packed = pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)
    y, _ = gru(packed)
    y, _ = pad_packed_sequence(y, batch_first=True, total_length=T)
    d_out = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    (y * d_out).sum().backward()

    sufs = ("", "_reverse")
    with torch.no_grad():
        gi = torch.stack([x @ getattr(gru, "weight_ih_l0" + s).t() + getattr(gru, "bias_ih_l0" + s) for s in sufs])
    whh = [getattr(gru, "weight_hh_l0" + s).detach() for s in sufs]
    bhh = [getattr(gru, "bias_hh_l0" + s).detach() for s in sufs]
    ref = GR.reference(gi, whh, bhh, lengths, d_out=d_out)
    assert ref.out.dtype == torch.float64
    assert float((ref.out - y.detach()).abs().max()) < 1e-13
    for d, s in enumerate(sufs):
        assert float((ref.g_bih[d] - getattr(gru, "bias_ih_l0" + s).grad).abs().max()) < 1e-12
        assert float((ref.g_bhh[d] - getattr(gru, "bias_hh_l0" + s).grad).abs().max()) < 1e-12
        # d W_ih = sum over frames of d gi^T x pins d gi itself (x is generic)
        dW = torch.einsum("btg,bti->gi", ref.d_g[d, :, :, :3].reshape(B, T, 3 * H), x)
        assert float((dW - getattr(gru, "weight_ih_l0" + s).grad).abs().max()) < 1e-12
        # d W_hh = sum d(gh)^T h_prev, d gh = (d a_r, d a_z, d q): pins the fourth block
        h = ref.out[:, :, d * H:(d + 1) * H]
        hprev = torch.zeros_like(h)
        if d == 0:
            hprev[:, 1:] = h[:, :-1]
        else:
            hprev[:, :-1] = h[:, 1:]
        dgh = torch.cat([ref.d_g[d, :, :, 0], ref.d_g[d, :, :, 1], ref.d_g[d, :, :, 3]], 2)
        dWhh = torch.einsum("btg,bth->gh", dgh, hprev)
        assert float((dWhh - getattr(gru, "weight_hh_l0" + s).grad).abs().max()) < 1e-12
    # frames past a clip's end: zero output, zero stash, zero gradient; the bias blocks are the column sums
    inv = ~ref.valid
    assert float(ref.out[inv].abs().max() if inv.any() else 0) == 0 and float(ref.d_g[:, inv].abs().sum()) == 0
    assert float(ref.save[:, inv].abs().sum()) == 0
    cs = ref.d_g.sum((1, 2))
    assert torch.allclose(ref.g_bhh, torch.cat([cs[:, 0], cs[:, 1], cs[:, 3]], 1), atol=1e-12, rtol=0)


def test_reference_stash_is_the_cell():
    """r, z, n, q of the stash rebuild the output: h = (1 - z) n + z h_prev, n = tanh(gi_n + r q)."""
    g = torch.Generator().manual_seed(3)
    B, T, H = 4, 5, 8
    lengths = torch.tensor([5, 1, 3, 4])
    gi = torch.randn(2, B, T, 3 * H, generator=g, dtype=torch.float64)
    whh = [torch.randn(3 * H, H, generator=g, dtype=torch.float64) * 0.3 for _ in range(2)]
    bhh = [torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1 for _ in range(2)]
    ref = GR.reference(gi, whh, bhh, lengths)
    for d in range(2):
        r, z, n, q = (ref.save[d, :, :, k] for k in range(4))
        h = ref.out[:, :, d * H:(d + 1) * H]
        hprev = torch.zeros_like(h)
        if d == 0:
            hprev[:, 1:] = h[:, :-1]
        else:
            hprev[:, :-1] = h[:, 1:]
        v = ref.valid[:, :, None].double()
        assert float((h - v * ((1 - z) * n + z * hprev)).abs().max()) < 1e-14
        assert float((v * (n - torch.tanh(gi[d, :, :, 2 * H:] + r * q))).abs().max()) < 1e-14
        assert float((v * (q - (hprev @ whh[d][2 * H:].t() + bhh[d][2 * H:]))).abs().max()) < 1e-14


def test_bf16_mode_rounds_where_the_kernels_do():
    """The bf16 mode is float32 with bf16 W_hh and bf16 previous state in the product: with operands that ARE bf16 numbers and
    T = 2 the forward equals the unrounded float32 recurrence except through the rounding of h_1; at T = 1 it equals it."""
    g = torch.Generator().manual_seed(5)
    B, H = 3, 8
    whh = [GR.bf(torch.randn(3 * H, H, generator=g) * 0.3) for _ in range(2)]
    bhh = [torch.randn(3 * H, generator=g) * 0.1 for _ in range(2)]
    gi = torch.randn(2, B, 1, 3 * H, generator=g)
    a = GR.reference(gi, whh, bhh, [1, 1, 1], bf16=True)
    b = GR.reference(gi, whh, bhh, [1, 1, 1], bf16=False)
    assert a.out.dtype == torch.float32 and float((a.out.double() - b.out).abs().max()) < 1e-6
    gi2 = torch.randn(2, B, 2, 3 * H, generator=g)
    a = GR.reference(gi2, whh, bhh, [2, 2, 1], bf16=True)
    b = GR.reference(gi2, whh, bhh, [2, 2, 1], bf16=False)
    err = float((a.out.double() - b.out).abs().max())
    assert 1e-6 < err < 2 ** -8 * H * 0.3 * 3  # the rounding of h_1 (2^-9 relative) through one row of W_hh, visible and small


# ------------------------------------------------------------------------------------------------------------ f32 dispatch
@pytest.mark.parametrize("H,B", sorted(GR.F32_EDGES_256))
def test_f32_dispatch_edges_at_256_cus(H, B):
    d = GR.f32_dispatch(B, 5, H, 256)
    assert (d.parts, d.sized_parts, d.pairs, d.grid_pairs, d.workgroups, d.part_major) == GR.F32_EDGES_256[(H, B)]
    assert (d.sync_bytes == 0) == (d.parts == 0)
    if d.parts:
        assert d.workgroups <= 240 and d.grid_pairs >= d.pairs
        # the pad is taken exactly when it fits
        pad = -(-d.pairs // 8) * 8
        assert d.grid_pairs == (pad if pad * d.parts <= 240 else d.pairs)
    # no workspace handed in: always the one-CU form
    assert GR.f32_dispatch(B, 5, H, 256, workspace=False).parts == 0
    # past the step-tag range the multi-CU form is off
    assert GR.f32_dispatch(B, 1023, H, 256).sync_bytes == 0 and GR.f32_dispatch(B, 1022, H, 256).sync_bytes == d.sync_bytes


def test_f32_dispatch_49_to_64_against_65():
    for B in range(49, 65):
        d = GR.f32_dispatch(B, 5, 192, 256)
        assert (d.pairs, d.grid_pairs, d.parts) == (8, 8, 12)
    d = GR.f32_dispatch(65, 5, 192, 256)
    assert d.grid_pairs - d.pairs == 6 and d.part_major


def test_f32_sync_bytes_literals():
    """SyncSections::bytes() = 64 header words + 8 bytes per granule; XCD ids [pairs][12] rounded up to 8, forward
    [2][pairs][16][H], backward [2][pairs][P][16][H] -- worked by hand for three shapes."""
    # B = 128, H = 192, twelve parts: 16 pairs -> 192 + 98 304 + 1 179 648 granules
    assert GR.f32_dispatch(128, 5, 192, 256).sync_bytes == 256 + 8 * (192 + 98304 + 1179648) == 10225408
    # B = 320, six parts: 40 pairs -> 480 + 245 760 + 1 474 560
    assert GR.f32_dispatch(320, 5, 192, 256).sync_bytes == 256 + 8 * (480 + 245760 + 1474560) == 13766656
    # B = 17, H = 64, two parts: 4 pairs -> 48 + 8 192 + 16 384
    assert GR.f32_dispatch(17, 5, 64, 256).sync_bytes == 256 + 8 * (48 + 8192 + 16384) == 197248
    # B = 1, twelve parts: 2 pairs, 24 ids
    assert GR.f32_dispatch(1, 5, 192, 256).sync_bytes == 256 + 8 * (24 + 12288 + 147456)


@pytest.mark.parametrize("B", [16, 128, 129])
def test_f32_cap_route_keeps_six_parts_in_a_twelve_part_workspace(B):
    free, cap = GR.f32_dispatch(B, 5, 192, 256), GR.f32_dispatch(B, 5, 192, 256, cap_set=True)
    assert cap.sync_bytes == free.sync_bytes and cap.sized_parts == free.sized_parts
    assert cap.parts == 6 and free.parts == (12 if B <= 128 else 6)
    assert cap.grid_pairs == {16: 8, 128: 16, 129: 24}[B] and cap.workgroups == cap.grid_pairs * 6


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("H", [192, 64])
def test_f32_dispatch_fits_and_is_monotone(cus, H):
    last_parts, seen_zero = None, False
    for B in range(1, 1300):
        for cap in (False, True):
            d = GR.f32_dispatch(B, 5, H, cus, cap_set=cap)
            assert d.workgroups <= cus - 16, (B, cap, d)
            if d.parts:
                assert d.workgroups == d.grid_pairs * d.parts and d.grid_pairs >= d.pairs
                assert d.parts <= d.sized_parts <= GR.SPLIT_MAX_PARTS
                # what a launch touches lies inside what the size query lays out, section by section
                for used, have in zip(GR.f32_launch_extent(d, H), GR.f32_sections(d, H)):
                    assert used <= have, (B, cap, d)
                assert d.sync_bytes == GR.sync_bytes(*GR.f32_sections(d, H))
        d = GR.f32_dispatch(B, 5, H, cus)
        if last_parts is not None:
            assert d.parts <= last_parts  # twelve -> six -> the one-CU form, never back
        last_parts = d.parts
        seen_zero |= d.parts == 0
        assert (d.sync_bytes > 0) == (d.parts > 0)
    assert seen_zero
    # more CUs never shrink the largest multi-CU batch
    largest = lambda c: max(B for B in range(1, 1300) if GR.f32_dispatch(B, 5, H, c).parts)
    assert largest(64) <= largest(256) <= largest(304)
    if cus == 256:
        assert largest(256) == (320 if H == 192 else 960)
    if cus == 64 and H == 192:  # 48 workgroups: twelve parts never fit (8 pairs x 12 = 96), six parts up to 8 pairs
        assert {GR.f32_dispatch(B, 5, H, 64).parts for B in range(1, 65)} == {6} and GR.f32_dispatch(65, 5, H, 64).parts == 0


# ------------------------------------------------------------------------------------------------------------ bf16 dispatch
@pytest.mark.parametrize("H,B", sorted(GR.BF16_EDGES_256))
def test_bf16_dispatch_edges_at_256_cus(H, B):
    d = GR.bf16_dispatch(B, 3, H, 256)
    assert d.launches == GR.BF16_EDGES_256[(H, B)]
    assert sum(nc for _, nc in d.launches) == B and all(c0 % 16 == 0 for c0, _ in d.launches)
    assert max(d.workgroups) <= 256
    P, groups = H // 64, 2 * -(-d.chunk // 16)
    assert d.sync_bytes == 256 + 8 * (-(-groups * P // 8) * 8 + groups * 16 * H + groups * P * P * 16 * 64)
    assert GR.bf16_dispatch(B, 1023, H, 256).chunk == 0


def test_bf16_dispatch_literals():
    # H = 512, B = 257: chunk 192 clips = 24 groups x 8 parts: 192 ids, 24 * 16 * 512 forward, 24 * 64 * 16 * 64 backward granules
    assert GR.bf16_dispatch(257, 3, 512, 256).sync_bytes == 256 + 8 * (192 + 196608 + 1572864)
    second = GR.bf16_dispatch(257, 3, 512, 256).launches[1]
    assert second == (192, 65) and -(-second[1] // 16) == 5 and second[1] % 16 == 1
    # unsupported widths and the step-kernel-only width
    assert GR.bf16_dispatch(16, 3, 1024, 256).chunk == 0 and GR.bf16_dispatch(16, 3, 64, 256).chunk == 0


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("H", [128, 256, 384, 512])
def test_bf16_dispatch_fits_and_covers(cus, H):
    single = []
    for B in range(1, 1400, 3):
        d = GR.bf16_dispatch(B, 3, H, cus)
        assert d.chunk > 0 and d.chunk % 16 == 0 or d.chunk == B
        assert max(d.workgroups) <= cus, (B, d)
        assert d.launches[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(d.launches, d.launches[1:]))
        assert d.launches[-1][0] + d.launches[-1][1] == B
        assert all(nc <= d.chunk for _, nc in d.launches)
        if len(d.launches) == 1:
            single.append(B)
    assert single == list(range(1, single[-1] + 1, 3))  # one launch up to a bound, several past it
