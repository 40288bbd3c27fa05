"""Child process of tests/test_gpu_data_parallel.py::test_one_rank_rccl_fit_equals_single_process.

Launched by ``python -m torch.distributed.run --nproc-per-node 1 ...`` BEFORE anything in this process has touched the GPU:
joins a one-rank "nccl" (= RCCL) group and runs the data-parallel ``harness.fit(plan="device", process_group=...)`` -- the
parameter broadcast, the gradient all-reduce of every step, the two metric collectives of every epoch, the barrier -- on the
clip directory the parent wrote, then leaves the log, the per-epoch history and ``best`` for the parent to compare."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(clip_dir: str, ckpt_path: str, out_path: str, epochs: int) -> None:
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    from silent_speech_amd import harness as Hn

    logs, history = [], []
    best = Hn.fit(clip_dir, ckpt_path, epochs=epochs, batch_size=16, patience=3, max_t=24, lr=3e-3, log=logs.append, plan="device",
                  rank=rank, world_size=world, process_group=dist.group.WORLD, history=history)
    torch.cuda.synchronize()
    torch.save({"best": best, "logs": logs, "history": history, "backend": dist.get_backend(), "world": world}, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]))
