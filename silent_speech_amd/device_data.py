"""Clips resident in HBM, batches assembled on the device.

Counterpart of ``NPZWordDataset`` + ``collate_fn`` (/root/reference/train_model_official.py:122-204) for the case the
reference cannot afford: every clip of the training set is uploaded ONCE (a ragged frame store: features
``(sum T, D)`` f32, ROI frames ``(sum Tr, H, W)`` u8) and a batch is two gather launches (``ss_batch_gather_f32`` /
``ss_batch_gather_u8``) driven by a ``(B, max_t)`` frame map.  The map encodes the reference's rules: noise on the
features with probability 0.7, one or two interior frames dropped from the FEATURES only (train...:146-152; the ROI
frames are not dropped), trim / zero-pad to ``max_t``, lengths aligned to ``min(T, Tr, max_t)``.

Three sources of randomness:
  * ``rng="reference"``: the host makes the draws with exactly the calls, order and distributions of the reference's
    ``__getitem__`` (``random.random``, ``np.random.normal``, ``random.randint``, ``np.random.choice``), so a batch is
    bit-identical to ``collate_fn([dataset[i] for i in indices])`` under the same seeds (tests/golden/dataset.npz);
  * ``rng="device"``: the decisions come from a ``numpy.random.Generator`` and the noise itself from the Philox stream
    inside the gather kernel -- nothing but two small index maps crosses PCIe;
  * ``rng="philox"``: the plan itself is made on the device (``ss_batch_plan``: one wave per batch row draws the
    decisions from the Philox stream and writes the maps, the lengths and the labels); with device indices from
    ``sample_epoch`` (``ss_epoch_sample``, the class-balanced sampler) nothing at all crosses PCIe and the host makes no
    per-clip step.  tests/batch_plan_ref.py restates both kernels in NumPy integers, bit for bit.

``AugmentPolicy`` (``batch(rng="philox", augment=True, policy=)``) adds what the reference's lineage had and its official
script dropped (inactive/train_reduced.py:103-123: time warp, scale jitter) and a per-clip shift of the ROI frames, planned and
applied on the device as well (``ss_batch_plan_aug``, ``ss_batch_gather_f32_aug``, ``ss_batch_gather_u8_shift``;
tests/aug_plan_ref.py restates them).  Without a policy the launches are the three above, unchanged.  The policy's masks (a masked
run of frames, a zeroed band of feature columns, a filled rectangle of the ROI frames) are two more launches when one of them is
on: ``ss_batch_plan_mask`` edits the maps behind either planner, ``ss_batch_mask_apply`` writes the band and the rectangle behind the
gathers.  Mixup (``mixup_prob`` > 0; inactive/train_reduced.py:36-53) is two more behind all of them: ``ss_batch_plan_mixup`` draws the
batch's factor and its partner rows, ``ss_batch_mixup`` writes the blended batch; tests/mixup_ref.py restates both.

In ``csrc/batch.hip`` the entry points are instantiations of a few kernels: ``ss_batch_plan`` / ``ss_batch_plan_aug`` of one plan
kernel (without / with the policy), ``ss_batch_gather_f32`` / ``_at`` / ``_aug`` of one feature gather (host-drawn or Philox noise,
the latter from any element offset of the stream, with or without the per-clip scale).  Here ``_batch_philox`` is the one
``rng="philox"`` path -- only its choice of entry points depends on the policy -- and ``_gather`` the one place that allocates
``X`` and ``R`` and launches the two gathers, for every rng.

Fine-tuning with the ROI CNN frozen (``Trainer(freeze_cnn=True)``): a frame's embedding depends on that frame and the CNN's weights
alone, so ``embed(model)`` runs the CNN over the store ONCE and ``batch(rng="philox", embedded=True)`` returns ``Z``, the rows
``features | embedding`` the GRU takes, from the unchanged plan kernel and one ``ss_batch_gather_z`` launch: 128 B of embedding per
frame instead of 4 096 B of pixels.  ``check()`` compares the CNN's parameters with the copy ``embed`` kept, so embeddings that
have gone stale are an error, not a silent one.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .data import DROP_FRAMES_MAX, DROP_FRAMES_PROB, MAX_T, NOISE_STD

NOISE_PROB = 0.7  # train...:144
_MASK64 = (1 << 64) - 1


def philox_noise_seed(seed: int, first_row: int) -> int:
    """Seed of the gather's feature-noise stream for the ``rng="philox"`` batch whose first row draws index ``first_row``:
    ``seed XOR ((first_row + 1) * 0x9E3779B97F4A7C15 mod 2^64)``.  The multiplier is odd, so distinct ``first_row`` values
    give distinct seeds: consecutive batches of an epoch never share a noise stream (the noise counter is the element
    index inside the batch, the same for every batch)."""
    return (int(seed) ^ (((int(first_row) + 1) * 0x9E3779B97F4A7C15) & _MASK64)) & _MASK64


@dataclass(frozen=True)
class AugmentPolicy:
    """Opt-in augmentations of the device-planned path, drawn per clip from the planner's Philox stream.

    ``time_warp_prob`` / ``time_warp_range``: a clip of more than 10 frames is re-timed to ``max(5, T * f)`` frames, ``f``
    uniform over the permille steps of the range; features and ROI frames follow the same warp (source frame
    ``j * (T - 1) // (L - 1)``); the reference's frame drop then acts on the warped clip.  ``scale_prob`` / ``scale_range``: the
    features (after the noise) times one factor uniform in the range.  ``roi_shift_prob`` / ``roi_shift_max`` = (dx, dy): the
    ROI frames of a clip moved by an integer offset uniform in [-dx, dx] x [-dy, dy], edges replicated (a crop box that
    jitters with the landmarks).

    The masks remove data where the three above move it (``ss_batch_plan_mask`` behind the planner, ``ss_batch_mask_apply`` behind the
    gathers; tests/mask_plan_ref.py restates both).  ``time_mask_prob`` / ``time_mask_max``: a clip of at least 8 planned frames gets
    one masked run of 1 .. ``min(time_mask_max, n // 4)`` frames inside ``[1, n)``; ``time_mask_streams`` = ``"both"``, ``"features"``
    or ``"roi"`` names the maps the run is written into, ``time_mask_fill`` = ``"zero"`` (zero rows; on the embedded path the
    embedding of a zero frame) or ``"hold"`` (the last frame before the run, repeated; the features still take fresh noise).
    ``feat_mask_prob`` / ``feat_mask_max``: one band of 1 .. ``min(feat_mask_max, D)`` feature columns set to 0.0 in every row of the
    clip.  ``cutout_prob`` / ``cutout_max`` = (w, h) / ``cutout_fill``: a clip with ROI frames gets one rectangle of at most w x h pixels
    filled with the grey level in all its frames (padding frames stay zero).  A mask is on when its probability is > 0 and its
    maximum >= 1; with all three off ``batch()`` issues the launches it issues without them.

    ``mixup_prob`` / ``mixup_alpha`` (the reference's lineage trains with it: inactive/train_reduced.py:36-53, 214-217): with
    probability ``mixup_prob`` a training batch, after everything above, is blended with a permutation of its own rows by one
    factor ``lam = k / 256`` per batch, ``k`` drawn from ``mixup_table(mixup_alpha)`` -- 1024 quantiles of Beta(alpha, alpha) in
    steps of 1 / 256.  Features ``fmaf(lam, X[b], (1 - lam) * X[perm[b]])``, ROI bytes ``(k R[b] + (256 - k) R[perm[b]] + 128) >> 8``,
    lengths the longer of the two; the partner labels and ``lam`` go to ``Trainer.step(mix=)``, whose loss is
    ``lam * CE(y) + (1 - lam) * CE(y[perm])``.  Off (``mixup_prob`` == 0) no launch is added."""
    time_warp_prob: float = 0.0
    time_warp_range: Tuple[float, float] = (0.8, 1.2)
    scale_prob: float = 0.0
    scale_range: Tuple[float, float] = (0.95, 1.05)
    roi_shift_prob: float = 0.0
    roi_shift_max: Tuple[int, int] = (0, 0)
    time_mask_prob: float = 0.0
    time_mask_max: int = 0
    time_mask_streams: str = "both"
    time_mask_fill: str = "zero"
    feat_mask_prob: float = 0.0
    feat_mask_max: int = 0
    cutout_prob: float = 0.0
    cutout_max: Tuple[int, int] = (0, 0)
    cutout_fill: int = 128
    mixup_prob: float = 0.0
    mixup_alpha: float = 0.2

    _STREAMS = ("both", "features", "roi")  # (the codes ss_batch_plan_mask takes: the position in the tuple)
    _FILLS = ("zero", "hold")

    def __post_init__(self):
        for name in ("time_warp_prob", "scale_prob", "roi_shift_prob", "time_mask_prob", "feat_mask_prob", "cutout_prob", "mixup_prob"):
            p = getattr(self, name)
            if not (isinstance(p, (int, float)) and 0.0 <= p <= 1.0):
                raise ValueError(f"{name} must lie in [0, 1], not {p!r}")
        for name in ("time_warp_range", "scale_range", "roi_shift_max", "cutout_max"):
            v = getattr(self, name)
            if not (isinstance(v, (tuple, list)) and len(v) == 2):
                raise ValueError(f"{name} must be a pair, not {v!r}")
            object.__setattr__(self, name, tuple(v))
        lo_pm, hi_pm = self.warp_permille()
        if not 0 < lo_pm <= hi_pm <= 4000:
            raise ValueError(f"time_warp_range must satisfy 0 < lo <= hi <= 4 (in steps of 0.001), not {self.time_warp_range!r}")
        lo, span = self.scale_lo_span()
        if not (np.isfinite(lo) and np.isfinite(span) and lo > 0 and self.scale_range[1] >= self.scale_range[0]):
            raise ValueError(f"scale_range must satisfy 0 < lo <= hi, not {self.scale_range!r}")
        mx, my = self.roi_shift_max
        if not all(isinstance(m, (int, np.integer)) and 0 <= m < 2 ** 30 for m in (mx, my)):
            raise ValueError(f"roi_shift_max must be two integers >= 0, not {self.roi_shift_max!r}")
        is_count = lambda m: isinstance(m, (int, np.integer)) and not isinstance(m, bool) and 0 <= m < 2 ** 31  # noqa: E731
        for name in ("time_mask_max", "feat_mask_max"):
            if not is_count(getattr(self, name)):
                raise ValueError(f"{name} must be an integer >= 0, not {getattr(self, name)!r}")
        if not all(is_count(m) for m in self.cutout_max):
            raise ValueError(f"cutout_max must be two integers >= 0, not {self.cutout_max!r}")
        if not (is_count(self.cutout_fill) and self.cutout_fill <= 255):
            raise ValueError(f"cutout_fill must be an integer in [0, 255], not {self.cutout_fill!r}")
        if self.time_mask_streams not in self._STREAMS:
            raise ValueError(f"time_mask_streams must be one of {self._STREAMS!r}, not {self.time_mask_streams!r}")
        if self.time_mask_fill not in self._FILLS:
            raise ValueError(f"time_mask_fill must be one of {self._FILLS!r}, not {self.time_mask_fill!r}")
        a = self.mixup_alpha
        if not (isinstance(a, (int, float)) and not isinstance(a, bool) and np.isfinite(a) and a > 0):
            raise ValueError(f"mixup_alpha must be a finite number > 0, not {a!r}")

    @classmethod
    def lineage(cls, **overrides) -> "AugmentPolicy":
        """The values of inactive/train_reduced.py:103-123 (warp 0.5 / 0.8-1.2, scale 0.3 / 0.95-1.05), no ROI shift."""
        return replace(cls(time_warp_prob=0.5, time_warp_range=(0.8, 1.2), scale_prob=0.3, scale_range=(0.95, 1.05)), **overrides)

    @property
    def time_mask_on(self) -> bool:
        return self.time_mask_prob > 0 and self.time_mask_max >= 1

    @property
    def feat_mask_on(self) -> bool:
        return self.feat_mask_prob > 0 and self.feat_mask_max >= 1

    @property
    def cutout_on(self) -> bool:
        return self.cutout_prob > 0 and min(self.cutout_max) >= 1

    @property
    def mixup_on(self) -> bool:
        return self.mixup_prob > 0

    def mixup_fields(self) -> dict:
        """``mixup_prob`` and ``mixup_alpha`` when mixup is on, else nothing: what ``harness.run_fingerprint`` adds for them."""
        return {name: float(getattr(self, name)) for name in MIXUP_FIELDS} if self.mixup_on else {}

    def mask_fields(self) -> dict:
        """The mask fields that differ from their defaults (tuples as lists): what ``harness.run_fingerprint`` adds for them, so
        the fingerprint of a policy that leaves the masks alone is what it was before they existed."""
        out = {}
        for name in MASK_FIELDS:
            v, default = getattr(self, name), type(self).__dataclass_fields__[name].default
            if v != default:
                out[name] = list(v) if isinstance(v, tuple) else v
        return out

    def mask_args(self, cutout: bool = True) -> tuple:
        """The policy's scalars as ``ss_batch_plan_mask`` takes them between ``seed`` and ``row_mask``.  ``cutout=False``: the cutout
        switched off (a store without ROI frames has no clip it could apply to)."""
        return (float(self.time_mask_prob), int(self.time_mask_max), self._STREAMS.index(self.time_mask_streams),
                self._FILLS.index(self.time_mask_fill), float(self.feat_mask_prob), int(self.feat_mask_max),
                float(self.cutout_prob) if cutout else 0.0, int(self.cutout_max[0]), int(self.cutout_max[1]), int(self.cutout_fill))

    def warp_permille(self) -> Tuple[int, int]:
        """The warp range as the planner takes it: integers, permille."""
        lo, hi = self.time_warp_range
        return int(round(float(lo) * 1000)), int(round(float(hi) * 1000))

    def scale_lo_span(self) -> Tuple[float, float]:
        """The scale range as the planner takes it: low end and hi - lo, each rounded to f32 once."""
        lo, hi = self.scale_range
        return float(np.float32(lo)), float(np.float32(float(hi) - float(lo)))


MASK_FIELDS = ("time_mask_prob", "time_mask_max", "time_mask_streams", "time_mask_fill", "feat_mask_prob", "feat_mask_max",
               "cutout_prob", "cutout_max", "cutout_fill")
MIXUP_FIELDS = ("mixup_prob", "mixup_alpha")


def mixup_table(alpha: float, N: int = 1024) -> np.ndarray:
    """-> (N,) uint16, ``k_i = round(256 * Q((i + 0.5) / N))`` with ``Q`` the quantile function of Beta(alpha, alpha): the table
    ``ss_batch_plan_mixup`` draws the batch's ``k`` from (``lam = k / 256``).  float64, NumPy alone.

    Beta(a, a) is symmetric about 1/2, so only ``x <= 1/2`` is computed: there the CDF is ``I(x) = B(x) / (2 B(1/2))``,
    ``B(x) = int_0^x t^(a-1) (1-t)^(a-1) dt``.  For ``a < 1``, with ``u = t^a`` the integrand becomes ``(1/a) (1 - u^(1/a))^(a-1)``
    on ``[0, (1/2)^a]``: bounded and smooth where the original has its ``t^(a-1)`` singularity.  For ``a >= 1`` there is no
    singularity, and a grid uniform in ``u`` would crowd into the last step before 1/2 as ``a`` grows (``(1/2)^a`` underflows in the
    end), so the grid is uniform in ``t`` and the integrand is ``(4 t (1-t))^(a-1)``, at most 1 for any ``a`` (the constant factor
    cancels in ``I``).  Composite Simpson gives ``B`` at the grid points, ``Q(p)`` for ``p <= 1/2`` is the linear inverse of that
    monotone table (the grid is fine enough that its error is far below the 1/512 that decides a rounding), and the upper half
    is the mirror image: ``k_i + k_(N-1-i) = 256``.  ``ValueError`` if the integral is not a positive finite number (an ``alpha``
    so small that ``1 / alpha`` overflows)."""
    a = float(alpha)
    if not (np.isfinite(a) and a > 0):
        raise ValueError(f"alpha must be a finite number > 0, not {alpha!r}")
    N = int(N)
    if N < 2 or N & (N - 1):
        raise ValueError(f"N must be a power of two >= 2, not {N!r}")
    M = 1 << 18  # Simpson panels (each of two half-steps)
    with np.errstate(all="ignore"):
        if a < 1.0:
            u = np.linspace(0.0, 0.5 ** a, 2 * M + 1)
            t = u ** (1.0 / a)
            f = (1.0 - t) ** (a - 1.0) / a
        else:
            u = t = np.linspace(0.0, 0.5, 2 * M + 1)
            f = (4.0 * t * (1.0 - t)) ** (a - 1.0)
        panels = (f[0:-1:2] + 4.0 * f[1::2] + f[2::2]) * ((u[2] - u[0]) / 6.0)
        cum = np.concatenate([[0.0], np.cumsum(panels)])  # B at t[0::2]
    if not (np.isfinite(cum[-1]) and cum[-1] > 0):
        raise ValueError(f"alpha {alpha!r}: the float64 integral of the Beta density is {cum[-1]!r}")
    cdf = cum / (2.0 * cum[-1])                       # 0 .. 1/2
    p = (np.arange(N // 2) + 0.5) / N
    x = np.interp(p, cdf, t[0::2])
    lo = np.floor(256.0 * x + 0.5).astype(np.int64)
    return np.concatenate([lo, 256 - lo[::-1]]).astype(np.uint16)


class DeviceClipStore:
    def __init__(self, files: Sequence[str], label_to_id, max_t: int = MAX_T, use_roi: bool = True, device="cuda"):
        L.load()
        self.max_t, self.device = max_t, torch.device(device)
        xs, rs, self.x_off, self.x_len, self.r_off, self.r_len, ys = [], [], [], [], [], [], []
        xo = ro = 0
        self.roi_hw = None
        for f in files:
            d = np.load(f, allow_pickle=True)
            X = d["X"].astype(np.float32)
            xs.append(X)
            self.x_off.append(xo)
            self.x_len.append(len(X))
            xo += len(X)
            ys.append(int(label_to_id[str(d["label"])]))
            if use_roi and "roi" in d.files:
                R = np.asarray(d["roi"], np.uint8)
                self.roi_hw = self.roi_hw or tuple(R.shape[1:])
                rs.append(R)
                self.r_off.append(ro)
                self.r_len.append(len(R))
                ro += len(R)
            else:
                self.r_off.append(-1)
                self.r_len.append(0)
        self.D = xs[0].shape[1]
        self.X = torch.from_numpy(np.concatenate(xs, 0)).to(self.device)
        self.R = torch.from_numpy(np.concatenate(rs, 0)).to(self.device) if rs else None
        if self.R is not None and (self.roi_hw[0] * self.roi_hw[1]) % 16:
            raise ValueError("ROI frames must be a multiple of 16 bytes")
        self.y = torch.tensor(ys, dtype=torch.int64, device=self.device)
        # rng="philox": the per-clip tables the planning kernels read, uploaded once
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)  # noqa: E731
        self._x_off_d, self._x_len_d = i32(self.x_off), i32(self.x_len)
        self._r_off_d, self._r_len_d = (i32(self.r_off), i32(self.r_len)) if self.R is not None else (None, None)
        # the sampler's tables: clip ids grouped by class (ascending class id, classes without clips left out)
        ya = np.asarray(ys, np.int64)
        present = np.unique(ya)
        self._members_d = i32(np.concatenate([np.flatnonzero(ya == c) for c in present]))
        self._class_start_d = i32(np.concatenate([[0], np.cumsum([(ya == c).sum() for c in present])]))
        self.n_classes_present = len(present)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)  # set by ss_batch_plan, read by check()
        self._plan_bufs = {}  # batch size -> (xmap, nmap, rmap, lens, y, row_scale, row_shift)
        self._mask_bufs = {}  # batch size -> row_mask (B, 8), for the batch sizes a policy with a mask on has planned
        self._mix_bufs = {}   # batch size -> (perm, y_b, lens_m, k, lam), for the batch sizes a policy with mixup on has planned
        self._mix_tables = {}  # mixup_alpha -> mixup_table(alpha) on the device, uploaded once
        self.mix = None  # (y_b, lam, perm, k) of the last batch a policy with mixup on has planned
        # embed(): the frozen CNN's embeddings of the ROI frames, of one all-zero frame, and what they were made from
        self.E = self.E0 = None
        self._embed_model = self._embed_params = self._embed_version = None

    def __len__(self):
        return len(self.x_len)

    # ------------------------------------------------------------------ decisions (host, a few integers per clip)
    def _plan(self, indices, augment, rng, gen):
        """Per clip: kept feature frames, whether noise is added (and, in reference mode, the noise itself)."""
        keeps, noises = [], []
        if rng == "reference":  # the reference's calls, in its order (train...:143-152)
            uniform, n_drop, choose = random.random, lambda: random.randint(1, DROP_FRAMES_MAX), np.random.choice
        else:
            uniform, n_drop, choose = gen.random, lambda: int(gen.integers(1, DROP_FRAMES_MAX + 1)), gen.choice
        for i in indices:
            T = self.x_len[i]
            keep = np.arange(T)
            noise = None
            if augment:
                if uniform() < 0.7:
                    noise = np.random.normal(0, NOISE_STD, size=(T, self.D)).astype(np.float32) if rng == "reference" else True
                if T > 12 and uniform() < DROP_FRAMES_PROB:  # mask out k interior frames: 0 and T-1 stay
                    m = np.ones(T, dtype=bool)
                    m[choose(np.arange(1, T - 1), size=n_drop(), replace=False)] = False
                    keep = keep[m]
            keeps.append(keep)
            noises.append(noise)
        return keeps, noises

    # ------------------------------------------------------------------ the plan made on the device (rng="philox")
    def sample_epoch(self, num_samples: Optional[int] = None, seed: int = 0, first: int = 0) -> torch.Tensor:
        """One epoch of the reference's ``WeightedRandomSampler(1 / count(label), replacement=True)`` (train...:382-397),
        drawn on the device: -> ``num_samples`` (default: one per clip) int32 clip ids.  Draw ``k`` of the result is draw
        ``first + k`` of the stream ``seed``: a data-parallel rank passes its offset and gets its shard of the same epoch."""
        n = len(self) if num_samples is None else int(num_samples)
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        L.call("ss_epoch_sample", self._members_d.data_ptr(), len(self), self._class_start_d.data_ptr(),
               self.n_classes_present, int(first) & _MASK64, n, int(seed) & _MASK64, out.data_ptr(), L.stream())
        return out

    def check(self) -> None:
        """Raises ``IndexError`` if a ``rng="philox"`` batch since the last call was given a device index outside the
        store (such a row comes back as an empty clip).  Reads one word back, so it synchronises: once per epoch, not per
        batch."""
        bad = int(self._err.item())
        if bad:
            self._err.zero_()
            raise IndexError("DeviceClipStore.batch(rng='philox'): a device index was outside [0, %d)" % len(self))
        if self._embed_model is not None:  # after embed(): the embeddings are those of the CNN as it is now
            now = self._embed_model.flat_params[:self._embed_params.numel()]
            if not torch.equal(now.to(self._embed_params.device), self._embed_params):
                raise RuntimeError("DeviceClipStore.check(): the model's ROI-CNN parameters have changed since embed(); the "
                                   "stored embeddings are stale (call embed(model) again, or train with freeze_cnn=True)")

    def embed(self, model, chunk: int = 8192) -> None:
        """Run ``model``'s ROI CNN over every ROI frame of the store, once: ``self.E`` (sum Tr, roi_emb) f32, ``self.E0``
        (roi_emb,) f32 = the embedding of one all-zero frame (what a clip without ROI frames stands for inside a ROI store: the
        pixel path hands the CNN zero frames, and the CNN of a zero frame is not zero).  ``model.embed_rois`` in chunks of ``chunk``
        frames -- the inference kernel, which treats every frame on its own.  A device copy of the CNN's parameters (the leading
        range of the flat bucket, ``model.cnn_param_range()``) and ``model._bucket_version`` are kept; ``check()`` raises once the
        parameters differ from the copy.  ``RuntimeError``: not an f32 ``use_roi`` model, a store without ROI frames, a ROI size
        outside the fused kernels' set."""
        from . import cnn_generic

        cfg = getattr(model, "cfg", None)
        if cfg is None or not cfg.use_roi or cfg.precision != "f32":
            raise RuntimeError("embed() needs an f32 use_roi model (the bf16 engine has no frozen-CNN path)")
        if self.R is None:
            raise RuntimeError("embed(): the store holds no ROI frames")
        if not cnn_generic.fused_supported(*self.roi_hw):
            raise RuntimeError("embed(): %dx%d ROI frames are outside the fused CNN kernels' set" % tuple(self.roi_hw))
        if model.flat_params.device != self.X.device:
            raise RuntimeError("embed(): the model and the store are on different devices")
        n, H, W = self.R.shape
        self.E = torch.empty(n, cfg.roi_emb, device=self.device, dtype=torch.float32)
        for lo in range(0, n, int(chunk)):
            hi = min(n, lo + int(chunk))
            model.embed_rois(self.R[lo:hi], out=self.E[lo:hi], ld_out=cfg.roi_emb)
        self.E0 = model.embed_rois(torch.zeros(1, H, W, device=self.device, dtype=torch.uint8)).reshape(-1)
        self._embed_model = model
        self._embed_params = model.flat_params[:model.cnn_param_range()].detach().clone()
        self._embed_version = model._bucket_version

    def empty_batch(self, embedded: bool = False):
        """A batch of no clips, shaped like ``batch()``'s: what a data-parallel rank hands ``Trainer.step`` when its shard of a
        global batch is empty (it still takes the step: the gradient all-reduce is collective).  ``embedded``: shaped like
        ``batch(embedded=True)``'s, for ``Trainer.step_embedded``."""
        dev, mt = self.device, self.max_t
        if embedded:
            if self.E is None:
                raise RuntimeError("empty_batch(embedded=True) needs a prior embed(model)")
            return (torch.empty(0, mt, self.D + self.E.shape[1], device=dev), torch.empty(0, dtype=torch.int64, device=dev), None,
                    torch.empty(0, dtype=torch.int64, device=dev))
        R = torch.empty((0, mt) + tuple(self.roi_hw), device=dev, dtype=torch.uint8) if self.R is not None else None
        return (torch.empty(0, mt, self.D, device=dev), torch.empty(0, dtype=torch.int64, device=dev), R,
                torch.empty(0, dtype=torch.int64, device=dev))

    def _gather(self, B, xmap, rmap, f32, shift=None):
        """Allocates ``X`` (and ``R`` when ``rmap`` is given) and launches the two gathers through the device maps.  ``f32``: the
        feature gather's entry point and its arguments between ``rows`` and ``dst``; ``shift``: those of ``ss_batch_gather_u8_shift``
        between ``rows`` and ``dst`` (``None``: the plain ``ss_batch_gather_u8``)."""
        mt, dev, s = self.max_t, self.device, L.stream()
        X = torch.empty(B, mt, self.D, device=dev)
        L.call(f32[0], self.X.data_ptr(), self.D, xmap.data_ptr(), B * mt, *f32[1:], X.data_ptr(), s)
        R = None
        if rmap is not None:
            H, W = self.roi_hw
            R = torch.empty(B, mt, H, W, device=dev, dtype=torch.uint8)
            if shift is None:
                L.call("ss_batch_gather_u8", self.R.data_ptr(), H * W, rmap.data_ptr(), B * mt, R.data_ptr(), s)
            else:
                L.call("ss_batch_gather_u8_shift", self.R.data_ptr(), H, W, rmap.data_ptr(), B * mt, *shift, R.data_ptr(), s)
        return X, R

    def _gather_z(self, B, xmap, rmap, tail):
        """Allocates ``Z`` (B, max_t, D + roi_emb) and fills it with ONE launch: features (noise and scale as the f32 gathers apply
        them, ``tail`` = ss_batch_gather_z's arguments between ``rows`` and ``dst``) | stored embeddings through ``rmap``."""
        mt, Eo = self.max_t, self.E.shape[1]
        Z = torch.empty(B, mt, self.D + Eo, device=self.device)
        L.call("ss_batch_gather_z", self.X.data_ptr(), self.D, xmap.data_ptr(), self.E.data_ptr(), Eo, rmap.data_ptr(),
               self.E0.data_ptr(), B * mt, *tail, Z.data_ptr(), self.D + Eo, L.stream())
        return Z

    def _batch_philox(self, indices, augment, seed, first_row, batch_first_row=None, policy=None, embedded=False):
        mt, dev = self.max_t, self.device
        if isinstance(indices, torch.Tensor) and indices.is_cuda:
            if indices.dtype != torch.int32 or indices.dim() != 1 or not indices.is_contiguous():
                raise ValueError("device indices must be a contiguous 1-D int32 tensor (a slice of sample_epoch())")
            idx_d = indices
        else:  # host indices are checked here, before anything is launched
            host = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else list(indices), dtype=np.int64).reshape(-1)
            if host.size and (host.min() < 0 or host.max() >= len(self)):
                raise IndexError("clip index outside [0, %d)" % len(self))
            idx_d = torch.from_numpy(host.astype(np.int32)).to(dev)
        B = idx_d.numel()
        if B == 0:
            raise ValueError("an empty batch")
        # rows [ahead, ahead + B) of the batch that starts at draw ``first``: that batch's noise stream, from this row on
        first = first_row if batch_first_row is None else batch_first_row
        ahead = int(first_row) - int(first)
        if ahead < 0:
            raise ValueError("batch_first_row lies behind first_row")
        if policy is not None and policy.mixup_on and (ahead or B > 1024):
            raise ValueError("mixup needs the whole batch (no shard of a larger one) and at most 1024 clips")
        noise_seed, noise_first = philox_noise_seed(seed, first), ahead * mt * self.D
        # One set of map / length / label buffers (and the policy's per-clip scale and shift) per batch size, reused by every
        # batch: the plan kernel, the two gathers and whatever consumes T and y afterwards are enqueued on L.stream() in order,
        # so the next plan overwrites them only after this batch's readers have run.  (T and y ARE these buffers: clone them to
        # keep them past the next call.)
        bufs = self._plan_bufs.get(B)
        if bufs is None:
            maps = torch.empty(3, B, mt, dtype=torch.int32, device=dev)
            bufs = self._plan_bufs[B] = (maps[0], maps[1], maps[2], torch.empty(B, dtype=torch.int64, device=dev),
                                         torch.empty(B, dtype=torch.int64, device=dev),
                                         torch.empty(B, dtype=torch.float32, device=dev),
                                         torch.empty(B, 2, dtype=torch.int32, device=dev))
        xmap, nmap, rmap, lens, y, row_scale, row_shift = bufs
        if self.R is None:
            rmap = None
        s = L.stream()
        head = (idx_d.data_ptr(), B, self._x_off_d.data_ptr(), self._x_len_d.data_ptr(), L.ptr(self._r_off_d), L.ptr(self._r_len_d),
                self.y.data_ptr(), len(self), mt, int(bool(augment)), int(first_row) & _MASK64, int(seed) & _MASK64, NOISE_PROB,
                float(DROP_FRAMES_PROB), int(DROP_FRAMES_MAX))
        outs = (xmap.data_ptr(), nmap.data_ptr(), L.ptr(rmap), lens.data_ptr(), y.data_ptr())
        if policy is None:
            L.call("ss_batch_plan", *head, *outs, self._err.data_ptr(), s)
            if augment and ahead:
                f32 = ("ss_batch_gather_f32_at", nmap.data_ptr(), float(NOISE_STD), noise_seed, noise_first)
            else:
                f32 = ("ss_batch_gather_f32", None, nmap.data_ptr() if augment else None, float(NOISE_STD) if augment else 0.0, noise_seed)
            shift = None
        else:
            (lo_pm, hi_pm), (sc_lo, sc_span), (mx, my) = policy.warp_permille(), policy.scale_lo_span(), policy.roi_shift_max
            if rmap is not None and (mx >= self.roi_hw[1] or my >= self.roi_hw[0]):
                raise ValueError("roi_shift_max %r does not fit %dx%d ROI frames" % ((mx, my), self.roi_hw[0], self.roi_hw[1]))
            L.call("ss_batch_plan_aug", *head, float(policy.time_warp_prob), lo_pm, hi_pm, float(policy.scale_prob), sc_lo, sc_span,
                   float(policy.roi_shift_prob), int(mx), int(my), *outs, row_scale.data_ptr(), row_shift.data_ptr(),
                   self._err.data_ptr(), s)
            f32 = ("ss_batch_gather_f32_aug", nmap.data_ptr(), float(NOISE_STD), noise_seed, noise_first, row_scale.data_ptr(), mt)
            shift = (row_shift.data_ptr(), mt, int(mx), int(my))
        # the masks: planned into the maps behind the planner, band and rectangle written behind the gathers (a policy whose masks
        # are all off adds no launch).  row_mask joins the per-batch-size buffers, reused in stream order like them.
        cutout = policy is not None and policy.cutout_on and rmap is not None
        band = policy is not None and policy.feat_mask_on
        row_mask = None
        if policy is not None and (policy.time_mask_on or band or cutout):
            row_mask = self._mask_bufs.get(B)
            if row_mask is None:
                row_mask = self._mask_bufs[B] = torch.empty(B, 8, dtype=torch.int32, device=dev)
            H, W = self.roi_hw if rmap is not None else (0, 0)
            L.call("ss_batch_plan_mask", xmap.data_ptr(), nmap.data_ptr(), L.ptr(rmap), lens.data_ptr(), B, mt, self.D, H, W,
                   int(bool(augment)), int(first_row) & _MASK64, int(seed) & _MASK64, *policy.mask_args(cutout), row_mask.data_ptr(), s)
        if embedded:  # the same plan, one gather: (noise_map, noise_std, seed, noise_first, row_scale, rows_per_clip)
            if policy is not None:
                tail = f32[1:]
            elif augment:
                tail = (nmap.data_ptr(), float(NOISE_STD), noise_seed, noise_first, None, 1)
            else:
                tail = (None, 0.0, noise_seed, 0, None, 1)
            Z = self._gather_z(B, xmap, rmap, tail)
            if band:
                L.call("ss_batch_mask_apply", Z.data_ptr(), Z.shape[2], self.D, None, 0, 0, None, row_mask.data_ptr(), B * mt, mt, 0, s)
            Z._ss_keep = (idx_d,)
            return Z, lens, None, y
        X, R = self._gather(B, xmap, rmap, f32, shift)
        if band or cutout:
            H, W = self.roi_hw if cutout else (0, 0)
            L.call("ss_batch_mask_apply", X.data_ptr() if band else None, self.D, self.D, R.data_ptr() if cutout else None, H, W,
                   rmap.data_ptr() if cutout else None, row_mask.data_ptr(), B * mt, mt, int(policy.cutout_fill), s)
        X._ss_keep = (idx_d,)
        if policy is not None and policy.mixup_on:
            return self._mixup(X, lens, R, y, B, augment, first, seed, policy)
        return X, lens, R, y

    def _mixup(self, X, lens, R, y, B, augment, batch_first_row, seed, policy):
        """Behind the gathers and the masks, on the same stream: ``ss_batch_plan_mixup`` (the batch's ``k``, ``perm``, the partners'
        labels, the longer lengths) and ``ss_batch_mixup`` (the blended ``X`` and ``R``, out of place).  The draw is keyed by the
        first row of the whole batch, so it is one per batch."""
        mt, dev, s = self.max_t, self.device, L.stream()
        table = self._mix_tables.get(float(policy.mixup_alpha))
        if table is None:
            host = mixup_table(policy.mixup_alpha).astype(np.int16)  # (entries <= 256: the same bits as uint16)
            table = self._mix_tables[float(policy.mixup_alpha)] = torch.from_numpy(host).to(dev)
        bufs = self._mix_bufs.get(B)
        if bufs is None:
            bufs = self._mix_bufs[B] = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev),
                                        torch.empty(B, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
                                        torch.empty(1, dtype=torch.float32, device=dev))
        perm, y_b, lens_m, k, lam = bufs
        L.call("ss_batch_plan_mixup", lens.data_ptr(), y.data_ptr(), B, int(bool(augment)), int(batch_first_row) & _MASK64,
               int(seed) & _MASK64, float(policy.mixup_prob), table.data_ptr(), table.numel(), perm.data_ptr(), y_b.data_ptr(),
               lens_m.data_ptr(), k.data_ptr(), lam.data_ptr(), s)
        Xm = torch.empty_like(X)
        Rm = None if R is None else torch.empty_like(R)
        fb = 0 if R is None else self.roi_hw[0] * self.roi_hw[1]
        L.call("ss_batch_mixup", X.data_ptr(), self.D, self.D, Xm.data_ptr(), L.ptr(R), L.ptr(Rm), fb, perm.data_ptr(),
               k.data_ptr(), B, mt, s)
        Xm._ss_keep = getattr(X, "_ss_keep", ())
        self.mix = (y_b, lam, perm, k)
        return Xm, lens_m, Rm, y

    def batch(self, indices: Sequence[int], augment: bool = False, rng: str = "device",
              generator: Optional[np.random.Generator] = None, seed: int = 0, first_row: int = 0,
              batch_first_row: Optional[int] = None, policy: Optional[AugmentPolicy] = None, embedded: bool = False):
        """-> X (B,max_t,D) f32, T (B,) i64, R (B,max_t,H,W) u8 or None, y (B,) i64 -- all on the device.

        ``rng="philox"``: the plan is made by ``ss_batch_plan`` on the device.  ``indices`` is a device int32 tensor (a
        slice of ``sample_epoch()``; out-of-range entries give empty rows and are reported by ``check()``) or a host
        sequence (validated here, ``IndexError`` before any launch).  Row ``b`` draws index ``first_row + b`` of the stream
        ``seed``: pass the position of the batch in the run so that no two batches share draws; the gather's noise seed is
        ``philox_noise_seed(seed, first_row)``.  ``batch_first_row`` (``rng="philox"`` only): these rows are rows
        ``first_row - batch_first_row`` onwards of a larger batch whose first row draws ``batch_first_row`` -- a data-parallel
        rank's shard of the global batch; the noise then continues that batch's stream, so the shards of all ranks,
        concatenated, are bit for bit the batch a single process assembles.  ``generator`` is not used.  ``R`` is returned whenever the store holds ROI
        frames (clips without ROI get zero frames, as ``collate_fn`` does when any clip of the batch has ROI); the
        per-batch "no clip has ROI -> ``R = None``" rule needs a read-back and is left to the host modes.  ``T`` and ``y``
        are buffers the store reuses for the next batch of the same size (safe in stream order; clone to keep them).

        ``policy`` (``rng="philox"`` with ``augment=True`` only, ``ValueError`` otherwise): an ``AugmentPolicy``; the batch is
        then planned and gathered by ``ss_batch_plan_aug`` / ``ss_batch_gather_f32_aug`` / ``ss_batch_gather_u8_shift``.  The
        decisions are keyed by the row's draw index like the rest of the plan, so shards (``batch_first_row``) stay bit-equal
        to the single-process batch.  ``None``: exactly the three launches described above.  A policy with a mask switched on (time
        mask, feature band, ROI cutout) adds ``ss_batch_plan_mask`` behind the planner and, for the band and the cutout,
        ``ss_batch_mask_apply`` behind the gathers; with all masks off neither is launched.  A policy with ``mixup_prob`` > 0 adds
        ``ss_batch_plan_mixup`` and ``ss_batch_mixup`` behind all of these: ``X``, ``T`` and ``R`` are then those of the blended batch
        (``T`` the longer of a row's and its partner's), ``y`` stays the rows' own labels, and ``self.mix`` = ``(y_b, lam, perm, k)``
        -- the partners' labels (B,) int64, the factor (1,) f32, the permutation (B,) int32 and ``k`` (1,) int32, all on the device and
        valid until the next ``batch`` call of that batch size -- is what ``Trainer.step(mix=(y_b, lam))`` takes.  The draw is keyed
        by the first row of the whole batch (``batch_first_row``); a shard of a larger batch would need its partners from other
        ranks, which is not built.  With ``mixup_prob`` == 0 the launches are those without the fields.

        ``embedded`` (``rng="philox"`` only, after ``embed(model)``): -> ``(Z, T, None, y)``, ``Z`` (B, max_t, D + roi_emb) f32 = the
        rows ``X | CNN(R)`` of the batch the same call returns without it (``model.forward_embedded(Z, T)`` are the logits of
        ``model(X, T, R)``), from the same plan kernel and ONE ``ss_batch_gather_z`` launch: the features take the same noise and
        scale bits, the embeddings are read from ``self.E`` through the ROI map (``self.E0`` where a clip has no ROI frames).  Time
        warp, scale jitter and the time mask act through the maps and the per-clip scale and work, and so does the feature band (on the
        first ``D`` columns of ``Z``; a zero-masked ROI row holds ``self.E0``); a policy with ``roi_shift_prob > 0`` or
        ``cutout_prob > 0`` is a ``ValueError``, since both act on pixels.  Without ``embedded`` the launches are exactly those described above."""
        if policy is not None:
            if not isinstance(policy, AugmentPolicy):
                raise TypeError("policy must be an AugmentPolicy")
            if rng != "philox" or not augment:
                raise ValueError("an AugmentPolicy needs rng='philox' and augment=True")
        if policy is not None and policy.mixup_on and embedded:
            raise ValueError("embedded=True cannot apply mixup_prob > 0: mixup of embedded batches is not built")
        if embedded:
            if rng != "philox":
                raise ValueError("embedded=True needs rng='philox': the embedded batch is planned on the device")
            if policy is not None and policy.roi_shift_prob > 0:
                raise ValueError("embedded=True cannot apply roi_shift_prob > 0: the shift acts on pixels, the store holds embeddings")
            if policy is not None and policy.cutout_prob > 0:
                raise ValueError("embedded=True cannot apply cutout_prob > 0: the cutout acts on pixels, the store holds embeddings")
            if self.E is None:
                raise RuntimeError("batch(embedded=True) needs a prior embed(model)")
        if rng == "philox":
            return self._batch_philox(indices, augment, seed, first_row, batch_first_row, policy, embedded)
        if batch_first_row is not None:
            raise ValueError("batch_first_row belongs to rng='philox'")
        indices = list(indices)
        B, mt = len(indices), self.max_t
        gen = generator or np.random.default_rng(seed)
        keeps, noises = self._plan(indices, augment, rng, gen)
        xmap = np.full((B, mt), -1, np.int32)
        nmap = np.full((B, mt), -1, np.int32)
        rmap = np.full((B, mt), -1, np.int32)
        lens = np.zeros(B, np.int64)
        host_noise: List[np.ndarray] = []
        n_rows = 0
        any_roi = self.R is not None and any(self.r_off[i] >= 0 for i in indices)
        for b, i in enumerate(indices):
            keep = keeps[b]
            t_eff = min(len(keep), mt)                                   # clip_pad_trim
            if any_roi and self.r_off[i] >= 0:
                t_eff = min(t_eff, self.r_len[i], mt)                     # T_use = min(T_eff, Tr, max_t)
                rmap[b, :t_eff] = self.r_off[i] + np.arange(t_eff)        # ROI frames are NOT dropped
            src = keep[:t_eff]
            xmap[b, :t_eff] = self.x_off[i] + src
            if noises[b] is not None:
                if rng == "reference":
                    nmap[b, :t_eff] = n_rows + src                       # noise was drawn for the undropped clip
                    host_noise.append(noises[b])
                    n_rows += self.x_len[i]
                else:
                    nmap[b, :t_eff] = 0
            lens[b] = t_eff
        dev = self.device
        xmap_d, nmap_d = torch.from_numpy(xmap).to(dev), torch.from_numpy(nmap).to(dev)
        rmap_d = torch.from_numpy(rmap).to(dev) if any_roi else None
        noise_d = torch.from_numpy(np.concatenate(host_noise, 0)).to(dev) if host_noise else None
        use_noise = augment and (noise_d is not None or rng != "reference")
        X, R = self._gather(B, xmap_d, rmap_d, ("ss_batch_gather_f32", L.ptr(noise_d), nmap_d.data_ptr() if use_noise else None,
                                                float(NOISE_STD) if (use_noise and noise_d is None) else 0.0,
                                                int(gen.integers(0, 2 ** 62)) if rng != "reference" else 0))
        # keep the maps alive until the launches have consumed them
        X._ss_keep = (xmap_d, nmap_d, noise_d)
        if R is not None:
            R._ss_keep = (rmap_d,)
        return X, torch.from_numpy(lens).to(dev), R, self.y[torch.as_tensor(indices, device=dev)]
