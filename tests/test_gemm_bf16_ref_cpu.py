"""The host references of tests/gemm_bf16_ref.py, pinned without a GPU: the rounding against torch's, the zones of ``place_bf16``
on a hand-checked operand, ``route_bf16`` around its thresholds, ``group_plan`` against a plan worked by hand and its invariants
over a sweep, and ``carry_free_rows`` against the true map."""
import numpy as np
import pytest
import torch

import gemm_bf16_ref as BR
import gemm_ref as GR
from gemm_ref import IDENT, Call

NAN16 = BR.BF16_NAN


def test_tie_table_holds_the_ties_the_issue_names():
    x = BR.tie_table()
    assert {257.0, 259.0, 1.0 + 2.0**-8, 1.0 - 2.0**-9}.issubset(set(x[np.isfinite(x)].tolist()))
    r = dict(zip(x.tolist(), BR.bf16_round(x).tolist()))
    assert r[257.0] == 256.0 and r[259.0] == 260.0 and r[1.0 + 2.0**-8] == 1.0 and r[1.0 + 3 * 2.0**-8] == 1.0 + 2.0**-6


def test_bf16_round_matches_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([BR.tie_table(), rng.integers(0, 2**32, size=2**16, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    bits = BR.bf16_bits(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert nan.sum() > 100 and (~nan).sum() > 60000
    assert np.array_equal(bits[~nan], want[~nan])
    got_f = BR.bf16_round(x)
    assert np.isnan(got_f[nan]).all() and np.isnan(BR.bf16_decode(want[nan])).all()
    assert got_f.dtype == np.float32 and bits.dtype == np.uint16
    assert np.array_equal(BR.bf16_bits(got_f[~nan]), bits[~nan])          # idempotent
    assert BR.bf16_round(np.array([np.inf, -np.inf], np.float32)).tolist() == [np.inf, -np.inf]
    assert BR.bf16_round(np.array([0x7F7F8000], np.uint32).view(np.float32))[0] == np.inf


@pytest.mark.parametrize("kc", [1, 0])
def test_place_bf16_zones(kc):
    """A 3 x 5 operand (3 rows of 5 k), ld = 8 + 8, two batch entries 8 elements apart, rows mapped r -> (r / 2) * 3 + r % 2 + 1."""
    rows, K = 3, 5
    R, W = (rows, K) if kc else (K, rows)
    vals = [np.arange(1, R * W + 1, dtype=np.float32).reshape(R, W) + 100 * b for b in range(2)]
    rmap = (2, 3, 1)
    buf, base, ld, stride = BR.place_bf16(kc, rows, K, 8, rmap, vals, gap=8)
    assert ld == 16 and base == 8 * 16
    sr = [1, 2, 4, 5, 7][:R]                       # storage rows of r = 0 ..: row 0, 3, 6 are skipped
    assert stride == (sr[-1] + 1) * 16 + 8
    assert buf.size == base + 2 * stride + 8 * 16
    zone = np.full(buf.size, "n")
    for b in range(2):
        for r, s in enumerate(sr):
            o = base + b * stride + s * ld
            assert np.array_equal(BR.bf16_decode(buf[o:o + W]), vals[b][r])
            zone[o:o + W] = "v"
            zone[o + W:o + 8] = "z"
    assert (buf[zone == "z"] == 0).all() and (buf[zone == "n"] == NAN16).all()
    assert (zone == "z").sum() == 2 * R * (8 - W) and (zone == "v").sum() == 2 * R * W
    # the guard rows, the skipped rows 0 and 3, the leading dimension behind column 8 and the gap are NaN
    assert (buf[:base] == NAN16).all() and (buf[base:base + ld] == NAN16).all() and (buf[base + 3 * ld:base + 4 * ld] == NAN16).all()
    assert (buf[base + ld + 8:base + 2 * ld] == NAN16).all() and (buf[base + stride - 8:base + stride] == NAN16).all()
    assert (buf[base + 2 * stride:] == NAN16).all()
    # the reference reads exactly the entries
    c = Call(kc, 1, rows, 1, K, ld, 8, 1, ra=rmap, flags=8, batch=2, stride_a=stride, stride_c=rows, a_base=base)
    ones = BR.bf16_bits(np.ones(8, np.float32))
    out, valid = BR.reference_bf16(c, buf, ones, np.zeros(2 * rows))
    opA = [v if kc else v.T for v in vals]
    assert np.array_equal(out.reshape(2, rows), np.stack([a.sum(1) for a in opA])) and valid.all()


def test_reference_bf16_rounds_an_f32_source_and_translates_flags():
    a = np.array([257.0, 259.0, 3.0, 1.0 + 2.0**-8], np.float32)      # [1][4] k-contiguous
    b = np.array([1.0, 1.0, 1.0, 1.0], np.float32)
    c = Call(1, 1, 1, 1, 4, 4, 4, 1, flags=1 | 4, bias_base=0)        # accumulate + atomics: bit 2 is no ReLU here
    out, valid = BR.reference_bf16(c, a, b, np.array([-1000.0]), np.array([0.5]))
    assert out[0] == 256.0 + 260.0 + 3.0 + 1.0 - 1000.0 + 0.5 and valid.all()
    out16, _ = BR.reference_bf16(Call(1, 1, 1, 1, 4, 8, 8, 1, flags=8), BR.bf16_bits(np.r_[a, 0, 0, 0, 0]), BR.bf16_bits(np.r_[b, 0, 0, 0, 0]),
                                 np.array([7.0]))
    assert out16[0] == 520.0
    with pytest.raises(AssertionError):
        BR.ref_call(Call(1, 1, 1, 1, 4, 4, 4, 1, flags=2))
    # the summed batch has one C and one bias
    a2, b2 = np.array([1.0, 2.0], np.float32), np.array([3.0, 5.0], np.float32)
    out, valid = BR.reference_bf16(Call(1, 1, 1, 1, 1, 4, 4, 1, flags=16, batch=2, stride_a=1, stride_b=1, stride_c=99, bias_base=0),
                                   a2, b2, np.array([7.0]), np.array([0.25]))
    assert out[0] == 13.25


ROUTE_TABLE = [
    # M, K, flags, splits -> name, nkt, splits, tiles
    (127, 64, 8, 1, "staged_b16", 1, 1, (1,)), (128, 64, 8, 1, "ring", 1, 1, (1,)), (128, 63, 8, 1, "staged_b16", 1, 1, (1,)),
    (128, 65, 8, 1, "staged_b16", 2, 1, (2,)), (127, 65, 8, 1, "staged_b16", 2, 1, (2,)), (127, 64, 8 | 16, 1, "ring_kcat", 1, 1, (1,)),
    (8, 128, 8 | 16, 1, "ring_kcat", 2, 1, (2,)), (128, 64, 8 | 16, 1, "ring_kcat", 1, 1, (1,)), (128, 64, 0, 1, "staged_f32", 2, 1, (2,)),
    (128, 64, 1, 2, "staged_f32", 2, 2, (1, 1)), (127, 63, 8, 1, "staged_b16", 1, 1, (1,)),
    (128, 320, 8 | 1, 4, "ring", 5, 4, (2, 2, 1, 0)), (128, 320, 8 | 1, 5, "ring", 5, 5, (1, 1, 1, 1, 1)),
    (128, 320, 8 | 1, 9, "ring", 5, 5, (1, 1, 1, 1, 1)), (128, 192, 8 | 1, 2, "ring", 3, 2, (2, 1)), (128, 128, 8 | 1, 2, "ring", 2, 2, (1, 1)),
    (64, 289, 8 | 1, 4, "staged_b16", 5, 4, (2, 2, 1, 0)), (64, 160, 1, 4, "staged_f32", 5, 4, (2, 2, 1, 0)),
]


@pytest.mark.parametrize("M,K,flags,splits,name,nkt,sp,tiles", ROUTE_TABLE)
def test_route_bf16(M, K, flags, splits, name, nkt, sp, tiles):
    r = BR.route_bf16(Call(1, 0, M, 8, K, BR.ceil8(K), 8, 8, flags=flags, splits=splits, batch=2))
    assert r == BR.RouteBf16(name, nkt, sp, tiles)


@pytest.mark.parametrize("nwg", list(range(1, 20)) + [255, 256, 257])
def test_xcd_contiguous_id_is_a_bijection(nwg):
    ids = [BR.xcd_contiguous_id(w, nwg) for w in range(nwg)]
    assert sorted(ids) == list(range(nwg))
    for x in range(8):   # an XCD's tiles are consecutive
        mine = [ids[w] for w in range(x, nwg, 8)]
        assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True


def test_group_plan_hand_worked():
    """cus = 4; problem 0: two tiles of 3 k tiles, problem 1: one tile of 4 -> 10 units, U = ceil(10 / 4) = 3, 4 workgroups,
    maxc = (4 - 1) / 3 + 2 = 3.  Units: 0-2 tile (0, 0) | 3-5 tile (0, 1) | 6-9 tile (1, 0)."""
    p = BR.group_plan([(8, 8, 192, 2), (8, 8, 256, 1)], 4)
    assert (p.units, p.U, p.workgroups, p.maxc, p.tiles) == (10, 3, 4, 3, 3)
    assert p.ws_floats == 3 * 3 * 256 * 128
    assert p.runs == [[(0, 0, 0, 3)], [(0, 1, 0, 3)], [(1, 0, 0, 3)], [(1, 0, 3, 1)]]
    assert p.slots == [[(0, 0)], [(1, 0)], [(2, 0)], [(2, 1)]]
    assert p.counts == [1, 1, 2]
    assert p.whole            # 3 tiles on 4 CUs: 2 * 3 >= 4 and 3 <= 4 -- the launch itself takes one workgroup per tile
    # the same group on 3 CUs: U = 4; workgroup 0 crosses from tile (0, 0) into (0, 1), workgroup 1 from problem 0 into 1
    p = BR.group_plan([(8, 8, 192, 2), (8, 8, 256, 1)], 3)
    assert (p.U, p.workgroups, p.maxc) == (4, 3, 2)
    assert p.runs == [[(0, 0, 0, 3), (0, 1, 0, 1)], [(0, 1, 1, 2), (1, 0, 0, 2)], [(1, 0, 2, 2)]]
    assert p.slots == [[(0, 0), (1, 0)], [(1, 1), (2, 0)], [(2, 1)]]
    assert p.counts == [1, 2, 2]


def test_group_plan_whole_thresholds():
    for cus in (4, 7, 256, 304):
        half = -(-cus // 2)
        for tiles, whole in ((half - 1, False), (half, True), (cus, True), (cus + 1, False)):
            if tiles >= 1:
                assert BR.group_plan([(8, 8, 128, tiles)], cus).whole == whole, (cus, tiles)


@pytest.mark.parametrize("cus", [1, 4, 7, 256, 304])
def test_group_plan_invariants(cus):
    rng = np.random.default_rng(cus)
    for _ in range(60):
        n = int(rng.integers(1, 9))
        probs = [(int(rng.choice([8, 256, 257, 520])), int(rng.choice([8, 128, 129, 260])), 64 * int(rng.integers(1, 13)),
                  int(rng.integers(1, 4))) for _ in range(n)]
        p = BR.group_plan(probs, cus)
        nkt = [K // 64 for _, _, K, _ in probs]
        ntile = [-(-M // 256) * -(-N // 128) * b for M, N, _, b in probs]
        assert p.units == sum(t * k for t, k in zip(ntile, nkt)) and p.tiles == sum(ntile)
        assert p.workgroups <= max(cus, 1) and p.workgroups == len(p.runs)
        seen = {}
        per_tile = {}
        for w, (runs, slots) in enumerate(zip(p.runs, p.slots)):
            assert sum(nk for *_, nk in runs) <= p.U
            for (j, tile, kt0, nk), (gt, slot) in zip(runs, slots):
                assert nk >= 1 and kt0 + nk <= nkt[j]
                assert 0 <= slot < p.maxc, "a slab outside the tile's slots"
                assert gt == sum(ntile[:j]) + tile
                per_tile.setdefault(gt, []).append(slot)
                for kt in range(kt0, kt0 + nk):
                    assert (j, tile, kt) not in seen
                    seen[(j, tile, kt)] = w
        assert len(seen) == p.units, "a unit is not covered"
        for gt in range(p.tiles):   # the reduce reads slots 0 .. cnt-1: exactly the ones written
            assert sorted(per_tile[gt]) == list(range(p.counts[gt])), (probs, gt)
        assert p.ws_floats == p.tiles * p.maxc * BR.SLAB_FLOATS


@pytest.mark.parametrize("rmap", [(5, 6, 1), (29, 30, 0), (7, 9, 2), (63, 64, 0), (65, 66, 1), (3, 4, 0)])
def test_carry_free_rows_differ_exactly_where_a_carry_is_due(rmap):
    G, S, off = rmap
    K = 64 * 6
    true, wrong = GR.map_rows(K, rmap), BR.carry_free_rows(K, rmap)
    assert np.array_equal(true[:64], wrong[:64])
    k = np.arange(K)
    # the carries due up to k's tile: the group boundaries crossed beyond the whole ones, one per 64-step at most
    due = (k // G) - ((k % 64) // G) - (k // 64) * (64 // G)
    assert np.array_equal(true - wrong, due * (S - G))
    assert (due[64:] > 0).any()
    # slices restart the exact division
    w2 = BR.carry_free_rows(K, rmap, starts=(0, 128))
    assert np.array_equal(w2[128:192], true[128:192]) and np.array_equal(w2[:128], wrong[:128])


def test_carry_free_rows_equal_the_map_when_the_group_divides_64():
    for rmap in [(8, 9, 1), (4, 5, 0), (2, 3, 0), (64, 65, 1)]:
        assert np.array_equal(BR.carry_free_rows(320, rmap), GR.map_rows(320, rmap))
    assert np.array_equal(BR.carry_free_rows(320, IDENT), np.arange(320))


def test_carry_matters_on_a_small_call():
    rmap_a, rmap_b = (5, 6, 1), (5, 6, 0)
    K, M, N = 320, 8, 8
    va = [GR.int_operands((K, M), 1)]
    vb = [GR.int_operands((K, N), 2)]
    a, a_base, lda, sa = BR.place_bf16(0, M, K, 0, rmap_a, va)
    b, b_base, ldb, sb = BR.place_bf16(0, N, K, 8, rmap_b, vb)
    c = Call(0, 0, M, N, K, lda, ldb, N, ra=rmap_a, rb=rmap_b, flags=8, a_base=a_base, b_base=b_base)
    assert BR.carry_matters(c, BR.bf16_decode(a), BR.bf16_decode(b))
    c8 = Call(0, 0, M, N, 64, lda, ldb, N, ra=rmap_a, rb=rmap_b, flags=8, a_base=a_base, b_base=b_base)
    assert not BR.carry_matters(c8, BR.bf16_decode(a), BR.bf16_decode(b))   # one k tile: nothing is stepped
