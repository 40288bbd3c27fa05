"""CPU: the host side of the data-parallel ``harness.fit`` -- the ABI of ``ss_eval_accum``, how ``epoch_shards`` cuts an epoch,
``top_confusions_from_matrix`` against ``top_confusions``, and ``reduce_epoch_metrics`` on two gloo ranks.

Every test here fails on a tree without the feature: the names do not exist there."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1


def test_the_library_declares_and_exports_ss_eval_accum():
    from silent_speech_amd import _lib

    txt = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = re.search(r"\bss_eval_accum\s*\(([^;]*)\)\s*;", txt)
    assert decl, "ss_eval_accum is not declared"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["ss_eval_accum"]) == 14
    lib = _lib.load()
    assert hasattr(lib, "ss_eval_accum")
    assert lib.ss_abi_version() == 3  # additive: no version bump
    # argument checks are host code: they answer without a GPU (nothing is launched)
    one = 1 << 20  # any non-NULL address: refused before it is used
    ok = [one, one, 4, 5, 0.05, 0, one, one, one, one, None, None, one, None]
    for pos in (0, 1, 6, 7, 8, 9, 12):  # every pointer but the two optional outputs
        args = list(ok)
        args[pos] = None
        assert lib.ss_eval_accum(*args) == -1, pos
    for pos, bad in ((2, 0), (2, -3), (3, 0), (3, -1), (5, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.ss_eval_accum(*args) == -1, (pos, bad)
    args = list(ok)
    args[2], args[5] = 4, I32_MAX - 3  # first_row + B = 2^31: past int32
    assert lib.ss_eval_accum(*args) == -1
    args[2], args[5] = I32_MAX, 1
    assert lib.ss_eval_accum(*args) == -1


@pytest.mark.parametrize("n,batch,world", [(n, b, w) for n in (45, 16) for b in (45, 16) for w in (1, 2, 3, 8)] + [(5, 16, 8)])
def test_epoch_shards_tile_every_global_batch(n, batch, world):
    from silent_speech_amd.harness import epoch_shards

    per_rank = [list(epoch_shards(n, batch, r, world)) for r in range(world)]
    steps = -(-n // batch)
    assert all(len(s) == steps for s in per_rank)  # every rank takes every step: the all-reduce is collective
    empty = 0
    for k in range(steps):
        g, g_end = k * batch, min(n, (k + 1) * batch)
        at = g
        for r in range(world):
            lo, hi, first_row, global_batch = per_rank[r][k]
            assert lo == at and lo <= hi <= g_end  # in rank order, nothing twice, nothing left out
            assert first_row == lo and global_batch == g_end - g
            empty += hi == lo
            at = hi
        assert at == g_end
    if (n, batch, world) == (5, 16, 8):
        assert empty == 3  # five rows over eight ranks: one each, three ranks idle
    if world == 1:
        assert [(lo, hi) for lo, hi, _, _ in per_rank[0]] == [(g, min(n, g + batch)) for g in range(0, n, batch)]


def test_epoch_shards_refuses_a_rank_outside_the_world():
    from silent_speech_amd.harness import epoch_shards

    for bad in ((45, 16, 2, 2), (45, 16, -1, 2), (45, 0, 0, 1), (45, 16, 0, 0)):
        with pytest.raises(ValueError):
            list(epoch_shards(*bad))


def matrices(y_true, y_pred, C, first_row=0):
    """What ss_eval_accum accumulates, in NumPy."""
    conf = np.zeros((C, C), np.int32)
    first = np.full((C, C), I32_MAX, np.int32)
    for b, (t, p) in enumerate(zip(y_true, y_pred)):
        conf[t, p] += 1
        first[t, p] = min(first[t, p], first_row + b)
    return conf, first


def test_top_confusions_from_matrix_equals_top_confusions():
    from silent_speech_amd.harness import top_confusions, top_confusions_from_matrix

    rng = np.random.default_rng(7)
    tied = 0
    for case in range(200):
        C = int(rng.integers(3, 8))
        n = int(rng.integers(0, 201))
        names = {i: "w%d" % i for i in range(C)}
        y_true = rng.integers(0, C, n).tolist()
        # few distinct errors, so that many cells share a count
        y_pred = [t if rng.random() < 0.5 else int(rng.integers(0, C)) for t in y_true]
        conf, first = matrices(y_true, y_pred, C)
        off = conf[~np.eye(C, dtype=bool)]
        tied += len(set(off[off > 0].tolist())) < (off > 0).sum()
        for k in (1, 6, 50):
            assert top_confusions_from_matrix(conf, first, names, k) == top_confusions(y_true, y_pred, names, k), (case, k)
    assert tied > 150  # the cases do exercise the tie rule
    # no errors at all, and no clips at all
    conf, first = matrices([0, 1, 2, 2], [0, 1, 2, 2], 3)
    assert top_confusions_from_matrix(conf, first, {0: "a", 1: "b", 2: "c"}, 6) == []
    assert top_confusions_from_matrix(*matrices([], [], 3), {0: "a", 1: "b", 2: "c"}, 6) == []
    # a tie is broken by the first occurrence, not by the cell's place in the matrix
    conf, first = matrices([2, 0, 2, 0], [1, 1, 1, 1], 3)
    assert top_confusions_from_matrix(conf, first, {0: "a", 1: "b", 2: "c"}, 6) == ["c→b(2)", "a→b(2)"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    rng = np.random.default_rng(11)
    C, n = 5, 37
    y_true = rng.integers(0, C, n)
    y_pred = np.where(rng.random(n) < 0.5, y_true, rng.integers(0, C, n))
    losses = rng.random(n).astype(np.float32)
    return C, n, y_true, y_pred, losses


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from silent_speech_amd import shard_range
    from silent_speech_amd.harness import reduce_epoch_metrics, top_confusions_from_matrix

    C, n, y_true, y_pred, losses = _case()
    lo, hi = shard_range(n, rank, world)
    conf, first = matrices(y_true[lo:hi], y_pred[lo:hi], C, first_row=lo)  # this rank's half, positions in the whole set
    sums = torch.tensor([float(losses[lo:hi].sum(dtype=np.float64)), float((y_true[lo:hi] == y_pred[lo:hi]).sum()), float(hi - lo)],
                        dtype=torch.float64)
    conf_t, first_t = torch.from_numpy(conf), torch.from_numpy(first)
    reduce_epoch_metrics(sums, conf_t, first_t, dist.group.WORLD)
    names = {i: "w%d" % i for i in range(C)}
    q.put((rank, sums.tolist(), conf_t.numpy().copy(), first_t.numpy().copy(),
           top_confusions_from_matrix(conf_t.numpy(), first_t.numpy(), names, 6)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_reduce_to_the_single_process_metrics():
    from silent_speech_amd.harness import reduce_epoch_metrics, top_confusions

    C, n, y_true, y_pred, losses = _case()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    conf, first = matrices(y_true, y_pred, C)
    want = top_confusions(y_true.tolist(), y_pred.tolist(), {i: "w%d" % i for i in range(C)}, 6)
    assert len(want) >= 3
    assert sorted(g[0] for g in got) == [0, 1]
    for _, sums, conf_r, first_r, strings in got:  # both ranks end with the whole set's metrics
        assert sums[2] == n and sums[1] == int((y_true == y_pred).sum())
        assert abs(sums[0] / n - float(losses.sum(dtype=np.float64)) / n) < 1e-12  # float64 sums of two halves
        assert np.array_equal(conf_r, conf) and np.array_equal(first_r, first) and conf_r.dtype == np.int32
        assert strings == want
    # without a group nothing happens at all
    sums, c, f = torch.ones(3, dtype=torch.float64), torch.from_numpy(conf.copy()), torch.from_numpy(first.copy())
    reduce_epoch_metrics(sums, c, f, None)
    assert sums.tolist() == [1, 1, 1] and np.array_equal(c.numpy(), conf) and np.array_equal(f.numpy(), first)


def test_fit_refuses_data_parallel_host_plans(tmp_path):
    from silent_speech_amd.harness import fit

    with pytest.raises(ValueError, match="plan='device'"):
        fit(str(tmp_path), str(tmp_path / "m.pt"), plan="host", rank=0, world_size=2)
    with pytest.raises(ValueError):
        fit(str(tmp_path), str(tmp_path / "m.pt"), plan="device", rank=2, world_size=2)
