"""CPU: the draws of ``gpu_support.write_clips`` are pinned, so that an edit to it cannot silently change the data under every ``fit``
test and under the recorded launch traces."""
import hashlib
import os

import numpy as np
import pytest

from gpu_support import WORDS, write_clips

# Recorded from ``write_clips`` of tests/test_gpu_data_parallel.py at the commit before the shared writer existed, run on the CPU
# with that file's two sets of arguments -- not from the shared writer.
PINNED = {
    "default": (dict(), "f5b6f9cd8f88973e0b2397a47cf6af7c1490297db3208e8593874ceb256eb2a9"),
    "landmarks_only": (dict(D=5, roi=None), "495eaf7b81b7740495ebaba77ed41c72bc3590266049635ca028d04f3a9d34ee"),
}


@pytest.mark.parametrize("case", list(PINNED))
def test_write_clips_recipe_is_pinned(tmp_path, case):
    """SHA-256 over, clip by clip in file order, the raw bytes of ``X``, those of ``roi`` where there is one, and the label; the
    constants come from the writer this one replaced (see PINNED), at n = 45, D = 20, roi = (32, 32) and at D = 5 without ROI."""
    kw, want = PINNED[case]
    d = write_clips(str(tmp_path / "clips_npz"), WORDS, **kw)
    names = sorted(os.listdir(d))
    assert names == [f"{k:03d}.npz" for k in range(45)]
    h = hashlib.sha256()
    for k, name in enumerate(names):
        with np.load(os.path.join(d, name), allow_pickle=False) as z:
            assert ("roi" in z.files) == (kw.get("roi", (32, 32)) is not None)
            assert z["X"].dtype == np.float32 and str(z["label"]) == WORDS[k % 3]
            h.update(z["X"].tobytes())
            if "roi" in z.files:
                assert z["roi"].dtype == np.uint8 and z["roi"].shape == (len(z["X"]), 32, 32)
                h.update(z["roi"].tobytes())
            h.update(str(z["label"]).encode())
    assert h.hexdigest() == want
