"""Helper of test_gpu_launch_trace.py: the ordered list of what one call hands to the device queues.

``traced(mp, model, fn)`` replaces ``_lib.call``, ``torch.cuda.Event.record`` and ``torch.cuda.Stream.wait_event`` for the length
of ``fn()`` (``mp``: a ``pytest.MonkeyPatch``) and returns the list:

    ["launch", entry point, timing tag, "main" | "side", [arguments]]    a kernel launch; "main" = its stream argument (the last
                                                                        one of every launcher) is the stream that was current when
                                                                        the call began.  Pointer-typed arguments (_lib.SIGNATURES)
                                                                        are "null" / "ptr", an ss_gemm_problem array is the list of
                                                                        its records (pointers marked the same way), everything
                                                                        else is the value
    ["record" | "wait", workspace attribute of the event, "main" | "side"]

``CASES`` are the model shapes of the test; ``run_case`` is what is traced of each.  Run as a program it records the traces of the
tree it is in:  python tests/launch_trace.py tests/launch_trace_parent.json
"""
import ctypes
import json
import os
import sys

import torch

T_F32 = 6
# name -> (constructor keywords, B, T, ROI size, traced calls)
CASES = {
    "f32_roi32": (dict(x_dim=84, num_classes=5, use_roi=True), 4, T_F32, (32, 32), ("step", "eval")),
    "f32": (dict(x_dim=84, num_classes=5), 4, T_F32, None, ("step", "eval", "autograd")),
    # B: the smallest batch without the multi-CU recurrence (the separate ss_dropout launch), asked of the library by the test
    "f32_one_cu": (dict(x_dim=84, num_classes=5), None, T_F32, None, ("step", "eval")),
    "bf16_grouped": (dict(x_dim=84, num_classes=5, hidden=128, gru_layers=3, precision="bf16"), 64, 4, None, ("step", "eval")),
    "bf16_three_launch": (dict(x_dim=84, num_classes=5, hidden=128, gru_layers=2, precision="bf16"), 12, 3, None, ("step", "eval")),
    "bf16_roi96": (dict(x_dim=84, num_classes=5, use_roi=True, roi_emb=64, hidden=128, precision="bf16",
                        cnn_channels=(16, 32, 64, 96)), 4, 3, (96, 96), ("step", "eval")),
}


def smallest_batch_without_gru_sync(T=T_F32, H=192, limit=4096):
    from silent_speech_amd import _lib

    return next(B for B in range(1, limit) if _lib.gru_sync_bytes(B, T, H) == 0)


def _mark(p):
    if isinstance(p, ctypes.c_void_p):
        p = p.value
    return "ptr" if p else "null"


def _argument(a, ctype):
    from silent_speech_amd import _lib

    if isinstance(a, ctypes.Array) and a._type_ is _lib.GemmProblem:
        return [{name: _mark(getattr(q, name)) if ft is ctypes.c_void_p else getattr(q, name) for name, ft in _lib.GemmProblem._fields_}
                for q in a]
    if ctype is ctypes.c_void_p:
        return _mark(a)
    return a


def traced(mp, model, fn):
    from silent_speech_amd import _lib

    torch.cuda.synchronize()
    main = torch.cuda.current_stream().cuda_stream
    log = []
    real_call, real_record, real_wait = _lib.call, torch.cuda.Event.record, torch.cuda.Stream.wait_event

    def which(handle):
        return "main" if (handle or 0) == main else "side"

    def call(name, *args, tag=None):
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), name
        has_stream = bool(sig) and sig[-1] is ctypes.c_void_p
        n = len(args) - 1 if has_stream else len(args)
        log.append(["launch", name, tag or name, which(args[-1]) if has_stream else "main",
                    [_argument(a, t) for a, t in zip(args[:n], sig[:n])]])
        return real_call(name, *args, tag=tag)

    def record(self, stream=None):
        log.append(["record", self, which((stream or torch.cuda.current_stream()).cuda_stream)])
        return real_record(self, stream)

    def wait_event(self, event):
        log.append(["wait", event, which(self.cuda_stream)])
        return real_wait(self, event)

    with mp.context() as m:
        m.setattr(_lib, "call", call)
        m.setattr(torch.cuda.Event, "record", record)
        m.setattr(torch.cuda.Stream, "wait_event", wait_event)
        fn()
    torch.cuda.synchronize()
    # (the events get their names afterwards: an autograd forward builds its workspace inside the traced call)
    names = {id(v): k for ws in model._ws_cache.values() for k, v in vars(ws).items() if isinstance(v, torch.cuda.Event)}
    for e in log:
        if e[0] != "launch":
            e[1] = names.get(id(e[1]), "?")
    return json.loads(json.dumps(log))  # tuples -> lists, as the recorded file has them


def launches(log):
    return [e for e in log if e[0] == "launch"]


def run_case(mp, name, side_stream):
    """-> {traced call: list}.  With ``side_stream`` off (both engines' USE_SIDE_STREAM) only the launches are kept."""
    import silent_speech_amd as ss
    from silent_speech_amd import engine, engine_bf16

    kw, B, T, hw, calls = CASES[name]
    if B is None:
        B = smallest_batch_without_gru_sync()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    X = torch.randn(B, T, kw["x_dim"], generator=g).to(dev)
    R = torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8).to(dev) if hw else None
    y = torch.randint(0, kw["num_classes"], (B,), generator=g).to(dev)
    # ragged: a clip shorter than T keeps walk_listed (an unsynchronised pinned read decides it for batches of full clips) fixed
    lengths = torch.tensor([max(1, T - b % 3) for b in range(B)], dtype=torch.int64, device=dev)
    out = {}
    with mp.context() as m:
        m.setattr(engine, "USE_SIDE_STREAM", side_stream)
        m.setattr(engine_bf16, "USE_SIDE_STREAM", side_stream)
        model = ss.BiGRUClassifier(**kw).to(dev).train()
        tr = ss.Trainer(model, dropout=True)
        tr.step(X, lengths, R, y)
        out["step"] = traced(mp, model, lambda: tr.step(X, lengths, R, y))
        model.eval()
        with torch.no_grad():
            out["eval"] = traced(mp, model, lambda: model(X, lengths, R))
        if "autograd" in calls:  # the d_X arm: d_X is cleared on the caller's stream and the d layer_in GEMM waits for ev_zero
            model.train()
            Xg = X.clone().requires_grad_()
            out["autograd"] = traced(mp, model, lambda: model(Xg, lengths, R).sum().backward())
        out["gru_sync"] = model._workspace(X, R, train=True, slot=0).gru_sync is not None
    assert sorted(out) == sorted(calls + ("gru_sync",))
    if not side_stream:
        out = {k: launches(v) if isinstance(v, list) else v for k, v in out.items()}
    return out


def key(name, side_stream):
    return f"{name}/{'side' if side_stream else 'one_stream'}"


def dumps(doc):
    """JSON with one trace entry per line: a launch that moved is one changed line of the file."""
    c = dict(separators=(",", ":"))
    cases = []
    for k, case in doc["traces"].items():
        parts = [f'  {json.dumps(n)}:' + ("[\n" + ",\n".join("   " + json.dumps(e, **c) for e in v) + "\n  ]" if isinstance(v, list)
                                          else json.dumps(v)) for n, v in case.items()]
        cases.append(f' {json.dumps(k)}:{{\n' + ",\n".join(parts) + "\n }")
    return '{"header":' + json.dumps(doc["header"], indent=1) + ',\n"traces":{\n' + ",\n".join(cases) + "\n}}\n"


if __name__ == "__main__":
    import pytest

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    mp = pytest.MonkeyPatch()
    doc = {"header": {"what": "launch and event traces of tests/test_gpu_launch_trace.py, recorded on one MI355X",
                      "recorded_with": "python tests/launch_trace.py tests/launch_trace_parent.json",
                      "tree": sys.argv[2] if len(sys.argv) > 2 else "unnamed",
                      "f32_one_cu_batch": smallest_batch_without_gru_sync()},
           "traces": {key(n, s): run_case(mp, n, s) for n in CASES for s in (True, False)}}
    with open(sys.argv[1], "w") as f:
        f.write(dumps(doc))
