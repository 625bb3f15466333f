"""Optimizer + LR schedule for the flat parameter store.

FlatSGD reproduces the hyper-parameter rules of /root/reference/solver/build.py:61-114 (`build_optimizer_C4`:
per-name LR factors REFINEMENT/MIL/DELTA, bias LR factor / weight decay) on top of torch.optim.SGD's update
(momentum, no dampening), executed by the fused `unit_sgd_momentum` kernel: one launch per contiguous
hyper-parameter segment of the flat buffer instead of one per tensor.

The two other things `build_optimizer_C4` does are honoured as well, on the device and without a host sync (csrc/optim.hip):
  * SOLVER.NESTEROV -- torch.optim.SGD(nesterov=True): b = momentum * b + d (first step b = d), p -= lr * (d + momentum * b);
  * SOLVER.CLIP_GRADIENTS (Detectron2's maybe_add_gradient_clipping; a cfg without the node means disabled). The clipped quantity is
    the true gradient g * grad_scale (data parallel: the all-reduced sum times 1 / world), before weight decay is added, as in torch.
      "value"       clamp(g * grad_scale, -CLIP_VALUE, CLIP_VALUE) per element; a NaN stays NaN.
      "norm"        per parameter tensor (one trainable FlatStore entry): norm = ||g * grad_scale||_p, p = NORM_TYPE in {1, 2, inf},
                    coef = min(1, CLIP_VALUE / (norm + 1e-6)); a non-finite norm gives a NaN coefficient for that tensor only
                    (torch's error_if_nonfinite=False); an all-zero gradient gives coef == 1.
      "full_model"  one coefficient for all trainable tensors, from the p-norm of the per-tensor norms. It needs every gradient before
                    any update: `step_tag` (EarlyUpdate) raises ValueError under it.
    One deviation from torch: the flat gradient buffer (`p.grad`) is LEFT UNCLIPPED -- the clip is fused into the update
    (`unit_sgd_step`), so the gradients are not written a second time. Padding elements of the flat buffer belong to no tensor and
    are updated as ever (coefficient 1).
    Under the norm types a step is one `unit_grad_clip_coefs` call per updated range (two launches for all its tensors) and then
    `unit_sgd_step` per hyper-parameter segment. `clip_coefs()` / `grad_norms()` return the device tensors of the last step: one
    float per trainable entry in `store.entries` order, `names` beside them; reading them involves no sync. With clipping disabled and
    NESTEROV false the launches are exactly the `unit_sgd_momentum` calls of before."""
import bisect

import torch

from . import ops


def hyper_for(cfg, name):
    s = cfg.SOLVER
    lr_mult, wd = 1.0, s.WEIGHT_DECAY
    module_name = name.rsplit(".", 1)[0]
    if name.endswith(".bias"):
        lr_mult *= s.BIAS_LR_FACTOR
        wd = s.WEIGHT_DECAY_BIAS
    if "oicr_predictors" in module_name or "regression_branch" in module_name:
        lr_mult *= s.REFINEMENT_LR_FACTOR
    if "classifier_stream" in module_name or "detection_stream" in module_name:
        lr_mult *= s.MIL_LR_FACTOR
    if "cls_score_delta" in module_name or "bbox_pred_delta" in module_name:
        lr_mult *= s.DELTA_LR_FACTOR
    return (lr_mult, wd)


CLIP_TYPES = ("value", "norm", "full_model")


def clip_config(cfg):
    """SOLVER.CLIP_GRADIENTS -> None (disabled, or a foreign cfg without the node) | (CLIP_TYPE, CLIP_VALUE, NORM_TYPE); an unknown
    CLIP_TYPE or NORM_TYPE is a ValueError whether or not the node is enabled"""
    node = getattr(cfg.SOLVER, "CLIP_GRADIENTS", None)
    if node is None:
        return None
    ctype, norm = getattr(node, "CLIP_TYPE", "value"), float(getattr(node, "NORM_TYPE", 2.0))
    if ctype not in CLIP_TYPES:
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE must be one of {CLIP_TYPES}, got {ctype!r}")
    if norm not in ops.NORM_KINDS:
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE must be 1.0, 2.0 or inf, got {norm!r}")
    if not getattr(node, "ENABLED", False):
        return None
    return (ctype, float(getattr(node, "CLIP_VALUE", 1.0)), norm)


def clip_table(store):
    """the trainable entries of a FlatStore as ([names], [(offset, numel)]) in `store.entries` order = ascending offsets, disjoint: the rows
    of the table the clipping kernels take"""
    ents = [e for e in store.entries if e["param"].requires_grad]
    rows = [(int(e["offset"]), int(e["numel"])) for e in ents]
    for (o0, n0), (o1, _) in zip(rows, rows[1:]):
        assert o0 + n0 <= o1, "FlatStore entries overlap or are out of order"
    assert not rows or (rows[0][0] >= 0 and rows[-1][0] + rows[-1][1] <= store.size)
    return [e["name"] for e in ents], rows


class WarmupMultiStepLR:
    """detectron2.solver.WarmupMultiStepLR (linear warm-up) as a pure function of the iteration."""

    def __init__(self, cfg):
        s = cfg.SOLVER
        self.base_lr, self.steps, self.gamma = s.BASE_LR, sorted(s.STEPS), s.GAMMA
        self.warmup_iters, self.warmup_factor = s.WARMUP_ITERS, s.WARMUP_FACTOR

    def __call__(self, it):
        f = 1.0
        if it < self.warmup_iters:
            alpha = it / self.warmup_iters
            f = self.warmup_factor * (1 - alpha) + alpha
        return self.base_lr * f * self.gamma ** bisect.bisect_right(self.steps, it)


class FlatSGD:
    def __init__(self, model, cfg, lr_schedule=None, grad_scale=1.0):
        self.model, self.cfg = model, cfg
        self.momentum = cfg.SOLVER.MOMENTUM
        self.nesterov = bool(getattr(cfg.SOLVER, "NESTEROV", False))
        if self.nesterov and self.momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")          # torch.optim.SGD's rule and words
        self.clip = clip_config(cfg)          # None | (type, value, norm type)
        self._clip_mode = ops.CLIP_NONE if self.clip is None else (ops.CLIP_VALUE if self.clip[0] == "value" else ops.CLIP_COEF)
        self.names = None         # names of the table's rows (set with the store)
        self._table = self._norms = self._coefs = self._clip_ws = None
        self.schedule = lr_schedule or WarmupMultiStepLR(cfg)
        self.iter = 0
        self.grad_scale = grad_scale
        self._store = None
        self._segments = None
        self._buf = None
        self._early = set()
        self._lr_dev = None       # device-resident learning rate (engine.GraphedStep): the launches then carry only the group multiplier

    def _bind(self):
        st = self.model.store
        if st is None or not st.is_current():
            st = self.model.flatten_parameters()
        if st is not self._store:
            self._store = st
            self._segments = st.segments(lambda n, p: hyper_for(self.cfg, n))
            self._buf = torch.zeros_like(st.params)
            self._first = True
            self.names, rows = clip_table(st)
            self._row_off = [o for o, _ in rows]
            self._row_end = [o + n for o, n in rows]
            self._chunk_prefix = [0]
            for _, n in rows:
                self._chunk_prefix.append(self._chunk_prefix[-1] + ops.clip_chunks(n))
            if self._clip_mode == ops.CLIP_COEF:          # everything a clipped step touches is allocated here, nothing inside a step
                dev = st.params.device
                self._table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(dev)
                self._norms = torch.zeros(len(rows), dtype=torch.float32, device=dev)
                self._coefs = torch.ones(len(rows), dtype=torch.float32, device=dev)
                self._clip_ws = ops.grad_clip_workspace(st.size, len(rows), dev)
        return st

    def _rows_in(self, lo, hi):
        """the table rows inside the flat range [lo, hi): bucket ranges (`store.tags`) and what is left between them hold whole tensors"""
        r0, r1 = bisect.bisect_left(self._row_off, lo), bisect.bisect_left(self._row_off, hi)
        assert (r0 == 0 or self._row_end[r0 - 1] <= lo) and (r1 == 0 or self._row_end[r1 - 1] <= hi), "an update range cuts a parameter tensor"
        return r0, r1

    def clip_coefs(self):
        """device float32 [len(names)]: the coefficients the last step multiplied each tensor's gradient by ("norm" / "full_model"; None
        otherwise). No sync: ordered on the current stream like `momentum_buffer()`."""
        self.join()
        return self._coefs

    def grad_norms(self):
        """device float32 [len(names)]: ||g * grad_scale||_p per tensor of the last step ("norm" / "full_model"; None otherwise)"""
        self.join()
        return self._norms

    def zero_grad(self, set_to_none=False):
        pass   # wgrad kernels overwrite the flat gradient buffer every step

    def _apply(self, st, lo, hi):
        """SGD-momentum on the flat range [lo, hi), cut at the hyper-parameter segment borders (solver/build.py:85-107 groups)"""
        lr = self.schedule(self.iter) if self._lr_dev is None else 1.0
        mode, value = self._clip_mode, (self.clip[1] if self.clip else 0.0)
        if mode == ops.CLIP_COEF:
            r0, r1 = self._rows_in(lo, hi)
            if r0 < r1:
                ops.grad_clip_coefs(st.grads, self._table, r0, r1, self._chunk_prefix[r1] - self._chunk_prefix[r0], self.clip[2], value,
                                    self.grad_scale, self._norms, self._coefs, self._clip_ws, full_model=self.clip[0] == "full_model")
        for off, n, (lr_mult, wd) in self._segments:
            a, b = max(off, lo), min(off + n, hi)
            if a >= b:
                continue
            if mode == ops.CLIP_NONE and not self.nesterov:
                ops.sgd_momentum(st.params[a:b], st.grads[a:b], self._buf[a:b], lr * lr_mult, self.momentum, wd,
                                 self.grad_scale, first_step=self._first, lr_dev=self._lr_dev)
            else:
                ops.sgd_step(st.params, st.grads, self._buf, a, b - a, lr * lr_mult, self.momentum, wd, self.grad_scale,
                             first_step=self._first, lr_dev=self._lr_dev, nesterov=self.nesterov, clip_mode=mode, clip_value=value,
                             table=self._table, coefs=self._coefs)

    def use_device_lr(self, device):
        """keep the scheduled learning rate in a device float that `write_lr()` refreshes (one tiny fill launch per step)"""
        if self._lr_dev is None:
            self._lr_dev = torch.zeros(1, dtype=torch.float32, device=device)
        self.write_lr()

    def write_lr(self):
        self._lr_dev.fill_(self.schedule(self.iter))

    def step_tag(self, tag):
        """update the parameters of one gradient bucket as soon as its gradients are final (called from the backward plan on the
        optimizer stream); `step()` then only covers what is left. Same kernel, same arithmetic, another launch partition.
        Under "norm" clipping a bucket's tensors are complete when the bucket is final (and, data parallel, all-reduced: the caller waits
        for the bucket first), so every rank computes the same coefficients with no extra collective."""
        if self.clip is not None and self.clip[0] == "full_model":
            raise ValueError('CLIP_TYPE "full_model" needs every gradient before any update: no per-bucket step_tag()')
        st = self._bind()
        for t, a, b in st.tags:
            if t == tag and (a, b) not in self._early:
                self._apply(st, a, b)
                self._early.add((a, b))

    def join(self):
        """make the current stream wait for an optimizer update that is still running on the model's weight-gradient stream
        (TrainerNoMeta(overlap_tail=True) / GeneralizedRCNN.overlap_optimizer_tail). Call it before reading `model.store.params`,
        `model.store.grads` or the momentum buffer on another stream between steps; `model.state_dict()`, `forward_train` and inference
        do so themselves. A no-op without a pending tail."""
        j = getattr(self.model, "join_optimizer_tail", None)
        if j is not None:
            j()

    def momentum_buffer(self):
        """the flat momentum buffer, safe to read on the current stream"""
        self.join()
        return self._buf

    def step(self):
        tail = getattr(self.model, "optimizer_tail", None)
        if tail is None:
            return self._step()
        with tail():          # the weight-gradient stream while the model overlaps the end of the step with the next one (rcnn.py)
            return self._step()

    def _step(self):
        st = self._bind()
        if self._early:
            done = sorted(self._early)
            lo = 0
            for a, b in done + [(st.size, st.size)]:
                if lo < a:
                    self._apply(st, lo, a)
                lo = max(lo, b)
            self._early = set()
        else:
            self._apply(st, 0, st.size)
        self._first = False
        self.iter += 1
        self.model.after_optimizer_step()


class MaskedFlatSGD(FlatSGD):
    """FlatSGD for the weak-only mode (engine.TrainerOnlyWeak, `train_only_weak=True`): torch leaves the .grad of a parameter no loss reaches
    at None and torch.optim.SGD skips it -- no weight decay, no momentum. FlatSGD sweeps the whole flat buffer, so a cleared range still
    decays; harmless for an occasional step without one batch, but in this mode the same tensors (RPN head, delta predictors, box_head of a
    two-head model) go without a gradient on EVERY iteration. Here the caller names, before every step, the trainable entries that received
    a gradient (`set_live(model.live_entries(...))`), and `unit_sgd_step_masked` neither read-modify-writes nor stores an element of a dead
    row; live rows and padding get `unit_sgd_step`'s result bit for bit. FlatSGD itself is untouched: a step that merely lacks one batch
    keeps its cleared, swept ranges.
    Dead rows need no first-step flag of their own: the momentum buffer starts at zero, so momentum * 0 + d == d is torch's buf = clone(d)
    on whichever step a tensor first becomes live. Under "norm" / "full_model" clipping the dead rows' gradients are the zeros the step
    cleared: their norms add nothing. `step_tag` (EarlyUpdate) and `step` go through the same `_apply`, so both follow the mask. The mask
    belongs to ONE step: `step()` consumes it, an update without one is an error, and so is a store that was re-flattened in between."""

    def __init__(self, model, cfg, lr_schedule=None, grad_scale=1.0):
        super().__init__(model, cfg, lr_schedule=lr_schedule, grad_scale=grad_scale)
        self._live = None         # tuple of bools, one per table row, for the step about to be applied; None = not set
        self._live_dev = self._live_store = self._mask_table = None

    def set_live(self, live):
        """live: one bool per trainable entry of the store (`clip_table` order), True = the step produced a gradient for it"""
        st = self._bind()
        live = tuple(bool(x) for x in live)
        if len(live) != len(self.names):
            raise ValueError(f"set_live: {len(live)} flags for the {len(self.names)} trainable tensors of the store")
        if self._mask_table is None or self._live_store is not st:
            rows = [(o, e - o) for o, e in zip(self._row_off, self._row_end)]
            self._mask_table = self._table if self._table is not None else torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(st.params.device)
        self._live, self._live_store = live, st
        # uploaded once per distinct mask (no host-to-device copy inside a step after the first of a kind)
        self._live_dev = self.model._const_on_device(("sgd_live", id(st), live), lambda: torch.tensor(live, dtype=torch.uint8))

    def _apply(self, st, lo, hi):
        if self._live is None:
            raise RuntimeError("MaskedFlatSGD: set_live() names the tensors with a gradient before every step (model.live_entries)")
        if self._live_store is not st:
            raise RuntimeError("MaskedFlatSGD: the parameter store was re-flattened after set_live(); the mask belongs to the old store")
        lr = self.schedule(self.iter) if self._lr_dev is None else 1.0
        mode, value = self._clip_mode, (self.clip[1] if self.clip else 0.0)
        if mode == ops.CLIP_COEF:
            r0, r1 = self._rows_in(lo, hi)
            if r0 < r1:
                ops.grad_clip_coefs(st.grads, self._table, r0, r1, self._chunk_prefix[r1] - self._chunk_prefix[r0], self.clip[2], value,
                                    self.grad_scale, self._norms, self._coefs, self._clip_ws, full_model=self.clip[0] == "full_model")
        for off, n, (lr_mult, wd) in self._segments:
            a, b = max(off, lo), min(off + n, hi)
            if a < b:
                ops.sgd_step_masked(st.params, st.grads, self._buf, a, b - a, lr * lr_mult, self.momentum, wd, self._mask_table, self._live_dev,
                                    self.grad_scale, first_step=self._first, lr_dev=self._lr_dev, nesterov=self.nesterov, clip_mode=mode,
                                    clip_value=value, coefs=self._coefs)

    def _step(self):
        super()._step()
        self._live = self._live_dev = None          # consumed: the next step names its own
