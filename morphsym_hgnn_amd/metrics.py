"""Step / epoch metrics of the reference's Lightning wrappers, computed on the MI355X through the C-ABI.

Mirrors the metric half of `Base_Lightning` (src/ms_hgnn/lightning_py/gnnLightning.py): `calculate_losses_step`
(:124-151, regression MSE / RMSE / L1; classification CE, 16-class accuracy, per-leg F1), `calculate_losses_epoch`
(:153-164), `reset_all_metrics` (:166-177), `classification_conversion_16_class` (:306-348) and
`body_frame_to_world_frame` (:663-676, which in the reference hops to the CPU and scipy every step).  The reference's
torchmetrics / customMetrics states are plain sums; here they live in two small device buffers that the kernels
`mshgnn_metrics_regression` / `mshgnn_metrics_classification` add into (include/mshgnn.h).  Same attribute names as the
reference (`mse_loss`, `rmse_loss`, `l1_loss`, `ce_loss`, `acc`, `f1_leg0..3`), values are float64 tensors.  As in the reference, the
loss a `training_step` returns (`mse_loss` / `ce_loss`, gnnLightning.py:709-722) carries autograd when `y_pred` does: its backward is one
launch of `mshgnn_mse_loss` / `mshgnn_ce_loss` (dL/dy_pred on the device), so a wrapper built on this class trains without torch's
elementwise loss kernels.

There is no CPU implementation: without a HIP device every method raises (`segmented_reference` / `com_segmented_reference`, the numpy mirrors the tests use as their yardstick, aside).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import engine as eng


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the MS-HGNN metrics run on a HIP device; there is no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f1(tp, fp, fn):
    """BinaryF1Score.compute (customMetrics.py:51-54), same operation order, float64; 0/0 -> 0 (nan_to_num)."""
    tp, fp, fn = tp.double(), fp.double(), fn.double()
    precision = tp / (tp + fp)
    recall = tp / (tp + fn)
    return torch.nan_to_num(2 * (precision * recall) / (precision + recall))


class _StepLoss(torch.autograd.Function):
    """The batch loss of `calculate_losses_step` as an autograd node.  forward: ONE launch -- this step's metric sums, the loss, their accumulation
    into the epoch state and dL/dy_pred (2 (y_pred - y) / n, or (softmax - onehot) / rows); backward: that gradient times the upstream scalar."""

    @staticmethod
    def forward(ctx, y_pred, y, metrics):
        buf, g = metrics._launch(y, y_pred, True)
        metrics._cur = buf          # (the sums are no autograd outputs: the only output is the loss the kernel left next to them)
        ctx.g, ctx.meta = g, (y_pred.shape, y_pred.dtype, y_pred.device)
        return buf[:8].view(torch.float64)[3 if metrics.regression else 2]

    @staticmethod
    def backward(ctx, gl):
        shape, dtype, in_dev = ctx.meta
        g = ctx.g * gl.to(ctx.g.device)           # (a 0-dim factor does not promote the fp32 gradient; out of place: backward may run twice)
        return g.to(device=in_dev, dtype=dtype).view(shape), None, None


class _RegStepLoss(torch.autograd.Function):
    """The L1 / Huber training loss of a regression step as an autograd node over `mshgnn_regression_loss` (one launch, bit-reproducible).  forward: the loss
    (fp32, 0-dim), keeping dL/dy_pred; backward: that gradient times the upstream scalar."""

    @staticmethod
    def forward(ctx, y_pred, y, metrics):
        loss, g = metrics._reg_launch(y, y_pred, True)
        ctx.g, ctx.meta = g, (y_pred.shape, y_pred.dtype, y_pred.device)
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        shape, dtype, in_dev = ctx.meta
        g = ctx.g * gl.to(ctx.g.device)
        return g.to(device=in_dev, dtype=dtype).view(shape), None, None


_REG_NAMES = ("mse_loss", "rmse_loss", "l1_loss")
_CLS_NAMES = ("ce_loss", "acc", "f1_leg0", "f1_leg1", "f1_leg2", "f1_leg3")


class StepMetrics:
    """Drop-in for the metric bookkeeping of `Base_Lightning` (`regression=True`: GRF / COM regression wrappers,
    `False`: contact classification).  The published values (`mse_loss`, ..., `f1_leg3`) are evaluated from the device sums when they are
    read, so a step that only needs its loss launches nothing for the others."""

    def __init__(self, regression: bool = True, device=None):
        self.regression = regression
        self.device = _device(device)
        self.lib = eng.load_library()
        # state layout (one buffer of 26 eight-byte words): [0:8] float64 -- regression: sq, abs, n | classification: ce, rows (a step's buffer also
        # holds the step's published values behind them, include/mshgnn.h); [8:26] int64 counts
        self._epoch = torch.zeros(26, dtype=torch.int64, device=self.device)
        self._scratch = torch.zeros(16384 // 8, dtype=torch.int64, device=self.device)      # MSHGNN_METRICS_SCRATCH_BYTES: partials + ticket
        self._cur = None          # the state the published values are read from: the last step's, or the epoch's
        self._loss = None         # the last step's loss when it carries autograd
        self._vals = {}
        self._from_step = False
        self.reg_loss = ("mse", 1.0)      # set_regression_loss: what `loss` (the value a training_step returns) is; the metric values never depend on it
        self._train = None                # the last step's L1 / Huber training loss
        self._train_args = None           # ... or what it is computed from when somebody reads `loss` (a step without autograd: validation, or a fused step about to publish its own)
        self._reg_scratch = None

    def set_regression_loss(self, kind: str, delta: float = 1.0) -> None:
        """The training loss of a regression wrapper: "mse" (the default: `loss` is `mse_loss`, everything as before), "l1" or "huber" with `delta`."""
        if not self.regression:
            raise ValueError("set_regression_loss: classification metrics (cross entropy)")
        eng.reg_loss_code(kind, delta)
        self.reg_loss, self._train, self._train_args = (kind, float(delta) if kind == "huber" else 1.0), None, None

    @property
    def _robust(self) -> bool:
        return self.regression and self.reg_loss[0] != "mse"

    @property
    def loss(self):
        """The training loss of the last step: `mse_loss` / `ce_loss`, or with set_regression_loss("l1" / "huber") that loss (after an epoch reduction there
        is none: `mse_loss`, the epoch's value, as with "mse")."""
        if not self.regression:
            return self.ce_loss
        if self._robust and self._train is None and self._train_args is not None:      # first read after a step without autograd: one launch, now
            self._train, self._train_args = self._reg_launch(*self._train_args, False)[0].view(()), None
        return self._train if self._robust and self._train is not None else self.mse_loss

    def _reg_launch(self, y: torch.Tensor, y_pred: torch.Tensor, want_grad: bool):
        dev = self.device
        yp = y_pred.detach().to(dev, torch.float32).flatten().contiguous()
        yy = y.detach().to(dev, torch.float32).flatten().contiguous()
        if yp.numel() != yy.numel():
            raise ValueError("y and y_pred must have the same number of elements")
        if self._reg_scratch is None:
            self._reg_scratch = torch.zeros(self.lib.mshgnn_regression_loss_scratch_bytes(1) // 8 + 1, dtype=torch.int64, device=dev)
        return eng.regression_loss(self.lib, dev, yp, yy, self.reg_loss[0], self.reg_loss[1], want_grad, self._reg_scratch)

    @property
    def _epoch_f(self):
        return self._epoch[:8].view(torch.float64)

    @property
    def _epoch_i(self):
        return self._epoch[8:]

    # ---- values from a state -----------------------------------------------------------------------------------
    def _names(self):
        return _REG_NAMES if self.regression else _CLS_NAMES

    def _value(self, name):
        if name not in self._names():
            raise AttributeError(f"'{name}' is not a metric of a {'regression' if self.regression else 'classification'} wrapper")
        if self._cur is None:
            return None
        if name in self._vals:
            return self._vals[name]
        f, i = self._cur[:8].view(torch.float64), self._cur[8:]
        if name in ("mse_loss", "ce_loss") and self._loss is not None:
            v = self._loss
        elif self._from_step:                              # the kernel left the step's values next to its sums: no launch
            v = f[(_REG_NAMES.index(name) + 3) if self.regression else (_CLS_NAMES.index(name) + 2)]
        elif name == "mse_loss":
            v = f[0] / f[2]
        elif name == "rmse_loss":
            v = torch.sqrt(f[0] / f[2])
        elif name == "l1_loss":
            v = f[1] / f[2]
        elif name == "ce_loss":
            v = f[0].float().double() / f[1]            # `summed_loss.float() / total_num`, customMetrics.py:24
        elif name == "acc":
            v = i[1].double() / i[0].double()
        else:
            k = int(name[-1])
            v = _f1(i[2 + 4 * k], i[3 + 4 * k], i[4 + 4 * k])
        self._vals[name] = v
        return v

    mse_loss = property(lambda self: self._value("mse_loss"))
    rmse_loss = property(lambda self: self._value("rmse_loss"))
    l1_loss = property(lambda self: self._value("l1_loss"))
    ce_loss = property(lambda self: self._value("ce_loss"))
    acc = property(lambda self: self._value("acc"))
    f1_leg0 = property(lambda self: self._value("f1_leg0"))
    f1_leg1 = property(lambda self: self._value("f1_leg1"))
    f1_leg2 = property(lambda self: self._value("f1_leg2"))
    f1_leg3 = property(lambda self: self._value("f1_leg3"))

    # ---- reference API -----------------------------------------------------------------------------------------
    def _launch(self, y: torch.Tensor, y_pred: torch.Tensor, want_grad: bool):
        """One launch: this batch's sums into a fresh state buffer, added into the epoch state, + dL/dy_pred (fp32) when asked for."""
        dev = self.device
        buf = torch.empty(26, dtype=torch.int64, device=dev)
        ep = self._epoch.data_ptr()
        with torch.cuda.device(dev):
            if self.regression:
                yp = y_pred.detach().to(dev, torch.float32).flatten().contiguous()
                yy = y.detach().to(dev, torch.float32).flatten().contiguous()
                if yp.numel() != yy.numel():
                    raise ValueError("y and y_pred must have the same number of elements")
                g = torch.empty_like(yp) if want_grad else None
                eng._check(self.lib, self.lib.mshgnn_metrics_regression_step(yp.data_ptr(), yy.data_ptr(), yp.numel(), buf.data_ptr(), ep,
                                                                             g.data_ptr() if want_grad else None, self._scratch.data_ptr(), _stream(dev)),
                           "mshgnn_metrics_regression_step")
            else:
                batch = y_pred.shape[0]
                yp = y_pred.detach().to(dev, torch.float32).reshape(batch * 4, 2).contiguous()     # gnnLightning.py:300
                yy = y.detach().to(dev, torch.int32).reshape(batch * 4).contiguous()
                g = torch.empty_like(yp) if want_grad else None
                eng._check(self.lib, self.lib.mshgnn_metrics_classification_step(yp.data_ptr(), yy.data_ptr(), batch, buf.data_ptr(), buf.data_ptr() + 64,
                                                                                 ep, ep + 64, g.data_ptr() if want_grad else None, self._scratch.data_ptr(),
                                                                                 _stream(dev)),
                           "mshgnn_metrics_classification_step")
        return buf, g

    def calculate_losses_step(self, y: torch.Tensor, y_pred: torch.Tensor):
        """Metrics of this batch (published as attributes) and accumulation into the epoch state.  When `y_pred` carries autograd, so does
        the published `mse_loss` / `ce_loss` -- what the reference's `training_step` returns for backward (gnnLightning.py:709-722)."""
        grad = torch.is_grad_enabled() and y_pred.requires_grad
        if grad and not self._robust:
            self._loss = _StepLoss.apply(y_pred, y, self)
        else:
            self._loss = None
            self._cur, _ = self._launch(y, y_pred, False)
        if self._robust:      # the metric values above are the metric kernel's at every kind; the training loss is a launch of its own -- with autograd now,
            # without (validation; a fused step, which publishes the engine's loss through set_step_loss) only if `loss` is read
            self._train, self._train_args = (_RegStepLoss.apply(y_pred, y, self), None) if grad else (None, (y.detach(), y_pred.detach()))
        self._vals, self._from_step = {}, True

    def set_step_loss(self, loss: torch.Tensor) -> None:
        """Publish `loss` (a differentiable scalar the caller computed for this step, e.g. the fused engine step's) as `mse_loss` / `ce_loss`; with
        set_regression_loss("l1" / "huber") as `loss` instead -- `mse_loss` stays the metric kernel's value."""
        if self._robust:
            self._train, self._train_args = loss, None
            return
        self._loss = loss
        self._vals.pop("mse_loss" if self.regression else "ce_loss", None)

    def calculate_losses_epoch(self) -> None:
        self._cur, self._loss, self._vals, self._from_step = self._epoch.clone(), None, {}, False
        self._train = self._train_args = None

    def reset_all_metrics(self) -> None:
        self._epoch.zero_()

    @staticmethod
    def classification_conversion_16_class(y_pred_per_foot_prob_only_1: torch.Tensor, y: torch.Tensor):
        """16-class probabilities and labels (gnnLightning.py:306-348) as tensors, vectorised: class j has bit (3 - k) of j
        set when foot k is in contact; P(j) = ((f0 f1)(f2 f3)) with f_k = p_k or 1 - p_k."""
        p = y_pred_per_foot_prob_only_1
        bits = torch.tensor([[(j >> (3 - k)) & 1 for k in range(4)] for j in range(16)], dtype=torch.bool, device=p.device)   # [16, 4]
        f = torch.where(bits.unsqueeze(0), p.unsqueeze(1), 1 - p.unsqueeze(1))                                               # [B, 16, 4]
        y_pred_new = (f[..., 0] * f[..., 1]) * (f[..., 2] * f[..., 3])
        w = torch.tensor([8, 4, 2, 1], dtype=torch.long, device=y.device)
        y_new = (y.long() * w).sum(dim=1, keepdim=True)
        return y_pred_new, y_new

    def body_frame_to_world_frame(self, batch_r_quat: torch.Tensor, grf_body_frame: torch.Tensor) -> torch.Tensor:
        """[N, 4] scalar-last world->body quaternions, [N, 12] body-frame GRFs -> [N, 12] world-frame GRFs, on device."""
        dev = self.device
        q = batch_r_quat.detach().to(dev, torch.float32).contiguous()
        g = grf_body_frame.detach().to(dev, torch.float32).contiguous()
        n = q.shape[0]
        if q.shape != (n, 4) or g.numel() != n * 12:
            raise ValueError("expected quaternions [N, 4] and 3-D GRFs [N, 12]")
        out = torch.empty(n, 12, dtype=torch.float32, device=dev)
        eng._check(self.lib, self.lib.mshgnn_grf_body_to_world(q.data_ptr(), g.data_ptr(), out.data_ptr(), n, _stream(dev)),
                   "mshgnn_grf_body_to_world")
        return out.to(grf_body_frame.dtype)


class ComStepMetrics(StepMetrics):
    """Metric bookkeeping of the centroidal-momentum wrappers (`COM_Base_Lightning`, gnnLightning_com.py:28-232): the regression values of
    `StepMetrics` (`mse_loss` differentiable, `rmse_loss`) plus `mse_loss_lin`, `mse_loss_ang`, `cos_sim_lin`, `cos_sim_ang`, `avg_cos_sim`
    and `loss` (`StepMetrics.loss`: `mse_loss`, as gnnLightning_com.py:121 has it, unless set_regression_loss chose L1 / Huber).  `y_mean` / `y_std`: the 6 label statistics of the dataset's `Standarizer` (soloDataset.py:12-46) --
    the cosine similarities are taken on base node 0 after un-standardising.  Two launches per step."""

    def __init__(self, num_bases: int, y_mean, y_std, device=None):
        super().__init__(regression=True, device=device)
        self.num_bases = int(num_bases)
        mean = [float(v) for v in torch.as_tensor(y_mean, dtype=torch.float64).flatten().tolist()]
        std = [float(v) for v in torch.as_tensor(y_std, dtype=torch.float64).flatten().tolist()]
        if len(mean) != 6 or len(std) != 6:
            raise ValueError("y_mean and y_std must have 6 entries (lin(3) | ang(3))")
        self._mean, self._std = (C.c_double * 6)(*mean), (C.c_double * 6)(*std)
        self._com_epoch = torch.zeros(8, dtype=torch.float64, device=self.device)
        self._com_cur = None
        self._com_scratch = torch.zeros(16384 // 8, dtype=torch.int64, device=self.device)

    def calculate_losses_step(self, y: torch.Tensor, y_pred: torch.Tensor):
        super().calculate_losses_step(y, y_pred)
        dev = self.device
        yp = y_pred.detach().to(dev, torch.float32).flatten().contiguous()
        yy = y.detach().to(dev, torch.float32).flatten().contiguous()
        per = self.num_bases * 6
        if yp.numel() != yy.numel() or yp.numel() % per:
            raise ValueError(f"y and y_pred must hold batch x {self.num_bases} x 6 values")
        cur = torch.empty(8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            eng._check(self.lib, self.lib.mshgnn_metrics_com_step(yp.data_ptr(), yy.data_ptr(), yp.numel() // per, self.num_bases, self._mean, self._std,
                                                                  cur.data_ptr(), self._com_epoch.data_ptr(), self._com_scratch.data_ptr(), _stream(dev)),
                       "mshgnn_metrics_com_step")
        self._com_cur = cur

    def calculate_losses_epoch(self) -> None:
        super().calculate_losses_epoch()
        self._com_cur = self._com_epoch.clone()

    def reset_all_metrics(self) -> None:
        super().reset_all_metrics()
        self._com_epoch.zero_()

    def _com(self, i, j):
        return None if self._com_cur is None else self._com_cur[i] / self._com_cur[j]

    mse_loss_lin = property(lambda self: self._com(0, 2))
    mse_loss_ang = property(lambda self: self._com(1, 3))
    cos_sim_lin = property(lambda self: self._com(4, 6))
    cos_sim_ang = property(lambda self: self._com(5, 6))
    avg_cos_sim = property(lambda self: None if self._com_cur is None else (self.cos_sim_lin + self.cos_sim_ang) / 2)
    # (`loss` is inherited: StepMetrics.loss)


# ---- per-segment sums: one row per (group element, sequence) out of one evaluation sweep ----------------------------------------------------------
# The reference's evaluators write one CSV row per symmetry operator with MSE / RMSE / L1 per test sequence (research/evaluator_regression-grf_c2.py:
# 170-221) or accuracy / per-leg F1 per operator (evaluator_classification_k4.py:57-89).  `SegmentedMetrics` keeps the sums of `StepMetrics` per segment
# id (mshgnn_metrics_regression_segmented / _classification_segmented, include/mshgnn.h): one launch per batch, deterministic, no host read until asked.

def _cls_terms(logits, labels):
    """Per-window classification terms in float64, operation by operation as the kernel's `met_cls_window`: (ce [B][4], counters int64 [B][18])."""
    import numpy as np
    lg = np.asarray(logits, dtype=np.float32).reshape(-1, 4, 2).astype(np.float64)
    lab = np.asarray(labels).reshape(-1, 4) != 0
    B = lg.shape[0]
    l0, l1 = lg[..., 0], lg[..., 1]
    m = np.maximum(l0, l1)
    e0, e1 = np.exp(l0 - m), np.exp(l1 - m)
    se = e0 + e1
    ce = (m + np.log(se)) - np.where(lab, l1, l0)
    p0, p1 = e0 / se, e1 / se
    pred = p1 > p0                                          # the first maximum wins
    c = np.zeros((B, 18), dtype=np.int64)
    for k in range(4):
        c[:, 2 + 4 * k] = pred[:, k] & lab[:, k]             # tp, fp, fn, tn
        c[:, 3 + 4 * k] = pred[:, k] & ~lab[:, k]
        c[:, 4 + 4 * k] = ~pred[:, k] & lab[:, k]
        c[:, 5 + 4 * k] = ~pred[:, k] & ~lab[:, k]
    v = np.empty((B, 16), dtype=np.float64)
    for j in range(16):
        f = [p1[:, k] if (j >> (3 - k)) & 1 else 1.0 - p1[:, k] for k in range(4)]
        v[:, j] = (f[0] * f[1]) * (f[2] * f[3])
    state = (lab.astype(np.int64) * np.array([8, 4, 2, 1])).sum(1)
    c[:, 0] = 1
    c[:, 1] = np.argmax(v, axis=1) == state                 # (np.argmax: the first maximum)
    return ce, c


def segmented_reference(y, y_pred, segment, n_segments: int, regression: bool = True):
    """Host mirror of one `SegmentedMetrics.update` (numpy; no GPU): the raw state the kernels would ADD, overflow row (index n_segments) included.
    The terms are formed in float64 with the kernels' operations, every sum is `math.fsum` (the correctly rounded sum of those terms), the
    integer counts are exact.  regression: float64 [n_segments + 1][3] (sq, abs, elements); classification: (float64 [n_segments + 1][2] (ce, rows),
    int64 [n_segments + 1][18])."""
    import math

    import numpy as np
    n_segments = int(n_segments)
    if n_segments < 1:
        raise ValueError("n_segments must be >= 1")
    B, groups = _segment_groups(segment, n_segments)
    to_np = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)
    if regression:
        yp = to_np(y_pred).astype(np.float32).reshape(B, -1).astype(np.float64)
        yy = to_np(y).astype(np.float32).reshape(B, -1).astype(np.float64)
        if yp.shape != yy.shape:
            raise ValueError("y and y_pred must have the same number of elements")
        d = yp - yy
        sq, ab = d * d, np.abs(d)
        state = np.zeros((n_segments + 1, 3), dtype=np.float64)
        for s, g in enumerate(groups):
            if g.size:
                state[s] = (math.fsum(sq[g].ravel()), math.fsum(ab[g].ravel()), float(g.size * yp.shape[1]))
        return state
    ce, c = _cls_terms(to_np(y_pred), to_np(y))
    ce_state = np.zeros((n_segments + 1, 2), dtype=np.float64)
    counts = np.zeros((n_segments + 1, 18), dtype=np.int64)
    for s, g in enumerate(groups):
        if g.size:
            ce_state[s] = (math.fsum(ce[g].ravel()), float(4 * g.size))
            counts[s] = c[g].sum(0)
    return ce_state, counts


def _segment_groups(segment, n_segments: int):
    """(batch, the window indices of every row 0 .. n_segments): an id outside [0, n_segments) belongs to the overflow row n_segments."""
    import numpy as np
    seg = np.asarray(segment.cpu() if isinstance(segment, torch.Tensor) else segment).astype(np.int64).reshape(-1)
    row = np.where((seg >= 0) & (seg < n_segments), seg, n_segments)
    order = np.argsort(row, kind="stable")
    bounds = np.searchsorted(row[order], np.arange(n_segments + 2))
    return seg.shape[0], [order[bounds[s]:bounds[s + 1]] for s in range(n_segments + 1)]


def com_window_terms(y, y_pred, num_bases: int, y_mean, y_std):
    """Per-window terms of the centroidal-momentum sums in float64, operation by operation as the kernels' `com_window_add` forms them (numpy: no fused
    multiply-add): (sq [B][num_bases][6] squared differences, cos [B][2] the cosines of base node 0's lin / ang vectors after un-standardising,
    sum (a / max(|a|, 1e-8)) (b / max(|b|, 1e-8)) with every sum of three in index order)."""
    import numpy as np
    to_np = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)
    nb = int(num_bases)
    yp = to_np(y_pred).astype(np.float32).reshape(-1, nb, 6).astype(np.float64)
    yy = to_np(y).astype(np.float32).reshape(-1, nb, 6).astype(np.float64)
    if yp.shape != yy.shape:
        raise ValueError("y and y_pred must hold batch x num_bases x 6 values")
    mean, std = np.asarray(y_mean, dtype=np.float64).reshape(6), np.asarray(y_std, dtype=np.float64).reshape(6)
    d = yp - yy
    cos = np.empty((yp.shape[0], 2), dtype=np.float64)
    for h in range(2):
        pv = yp[:, 0, 3 * h:3 * h + 3] * std[3 * h:3 * h + 3] + mean[3 * h:3 * h + 3]
        yv = yy[:, 0, 3 * h:3 * h + 3] * std[3 * h:3 * h + 3] + mean[3 * h:3 * h + 3]
        pp = (pv[:, 0] * pv[:, 0] + pv[:, 1] * pv[:, 1]) + pv[:, 2] * pv[:, 2]
        yq = (yv[:, 0] * yv[:, 0] + yv[:, 1] * yv[:, 1]) + yv[:, 2] * yv[:, 2]
        pn, yn = np.maximum(np.sqrt(pp), 1e-8), np.maximum(np.sqrt(yq), 1e-8)
        t = (pv / pn[:, None]) * (yv / yn[:, None])
        cos[:, h] = (t[:, 0] + t[:, 1]) + t[:, 2]
    return d * d, cos


def com_segmented_reference(y, y_pred, segment, n_segments: int, num_bases: int, y_mean, y_std):
    """Host mirror of one `SegmentedComMetrics.update` (numpy; no GPU), beside `segmented_reference`: the raw state float64 [n_segments + 1][8] the kernel
    would ADD, overflow row included, in the layout of mshgnn_metrics_com_step -- [0] / [1] squared error of the lin / ang halves, [2] = [3] =
    3 num_bases windows, [4] / [5] the cosine sums, [6] windows, [7] 0.  Terms: `com_window_terms`; every sum is `math.fsum`."""
    import math

    import numpy as np
    n_segments, nb = int(n_segments), int(num_bases)
    if n_segments < 1 or nb < 1:
        raise ValueError("n_segments and num_bases must be >= 1")
    B, groups = _segment_groups(segment, n_segments)
    sq, cos = com_window_terms(y, y_pred, nb, y_mean, y_std)
    if sq.shape[0] != B:
        raise ValueError("one segment id per window")
    state = np.zeros((n_segments + 1, 8), dtype=np.float64)
    for s, g in enumerate(groups):
        if g.size:
            n3 = float(3 * nb * g.size)
            state[s] = (math.fsum(sq[g][:, :, :3].ravel()), math.fsum(sq[g][:, :, 3:].ravel()), n3, n3, math.fsum(cos[g, 0]), math.fsum(cos[g, 1]),
                        float(g.size), 0.0)
    return state


def com_table_from_state(state):
    """The published values per segment from raw centroidal-momentum sums [..., 8] (torch float64, any device; the overflow row already cut off): `MSE`
    (= ([0] + [1]) / ([2] + [3]): the mean over all 6 num_bases values), `MSE_lin`, `MSE_ang`, `cos_sim_lin`, `cos_sim_ang`, `avg_cos_sim`, `n` (windows).
    An empty segment's means are NaN (0 / 0)."""
    lin, ang = state[..., 4] / state[..., 6], state[..., 5] / state[..., 6]
    return {"MSE": (state[..., 0] + state[..., 1]) / (state[..., 2] + state[..., 3]), "MSE_lin": state[..., 0] / state[..., 2],
            "MSE_ang": state[..., 1] / state[..., 3], "cos_sim_lin": lin, "cos_sim_ang": ang, "avg_cos_sim": (lin + ang) / 2, "n": state[..., 6]}


_SEG_REG_COLUMNS = ("MSE", "RMSE", "L1", "n")
_SEG_CLS_COLUMNS = ("CE", "accuracy", "f1_leg_0", "f1_leg_1", "f1_leg_2", "f1_leg_3", "f1_avg_legs", "n")


def table_from_state(state, counts=None, per_window: int = 1):
    """The published values per segment from raw sums (torch float64 / int64 tensors, any device; the overflow row already cut off):
    regression (counts None) `MSE`, `RMSE`, `L1`, `n`; classification `CE`, `accuracy`, `f1_leg_0..3`, `f1_avg_legs`, `n`.  `n` is the number
    of WINDOWS of the segment.  An empty segment's means are NaN (0 / 0); F1 follows the reference's 0 / 0 -> 0 (customMetrics.py:51-54)."""
    if counts is None:
        mse = state[:, 0] / state[:, 2]
        return {"MSE": mse, "RMSE": torch.sqrt(mse), "L1": state[:, 1] / state[:, 2], "n": state[:, 2] / float(per_window)}
    out = {"CE": state[:, 0].float().double() / state[:, 1],            # `summed_loss.float() / total_num`, customMetrics.py:24
           "accuracy": counts[:, 1].double() / counts[:, 0].double()}
    legs = [_f1(counts[:, 2 + 4 * k], counts[:, 3 + 4 * k], counts[:, 4 + 4 * k]) for k in range(4)]
    for k in range(4):
        out[f"f1_leg_{k}"] = legs[k]
    out["f1_avg_legs"] = (legs[0] + legs[1] + legs[2] + legs[3]) / 4.0
    out["n"] = counts[:, 0].double()
    return out


class SegmentedMetrics:
    """The sums of `StepMetrics` per segment: `update(y, y_pred, segment)` adds every window's sums to the row its id names, in ONE launch, bit-reproducibly
    (no floating-point atomic; include/mshgnn.h).  An id outside [0, n_segments) lands in an extra overflow row that `overflow()` / `check()` read."""

    def __init__(self, n_segments: int, regression: bool = True, device=None):
        if int(n_segments) < 1:
            raise ValueError("n_segments must be >= 1")
        self.n_segments, self.regression = int(n_segments), bool(regression)
        self.device = _device(device)
        self.lib = eng.load_library()
        if not hasattr(self.lib, "mshgnn_metrics_regression_segmented"):
            raise eng.MshgnnError("this build of the library has no mshgnn_metrics_regression_segmented / _classification_segmented")
        self.state = torch.zeros(self.n_segments + 1, 3 if regression else 2, dtype=torch.float64, device=self.device)
        self.counts = None if regression else torch.zeros(self.n_segments + 1, 18, dtype=torch.int64, device=self.device)
        self.per_window = 1 if regression else 4
        self._scratch, self._scratch_batch = None, 0

    def reserve(self, batch: int) -> None:
        """The scratch for batches of up to `batch` windows (`update` grows it when needed; reserve before capturing `update` in a graph)."""
        if batch > self._scratch_batch:
            nbytes = int(self.lib.mshgnn_metrics_segmented_scratch_bytes(int(batch)))
            self._scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=self.device)      # zeroed once; the calls own it from here
            self._scratch_batch = int(batch)

    def update(self, y: torch.Tensor, y_pred: torch.Tensor, segment: torch.Tensor) -> None:
        """y / y_pred as `calculate_losses_step` takes them, segment: int32 [batch] on the device (one id per window)."""
        dev = self.device
        seg = segment.detach().to(dev, torch.int32).reshape(-1).contiguous()
        batch = int(seg.numel())
        if batch < 1:
            raise ValueError("no windows")
        self.reserve(batch)
        with torch.cuda.device(dev):
            if self.regression:
                yp = y_pred.detach().to(dev, torch.float32).reshape(-1).contiguous()
                yy = y.detach().to(dev, torch.float32).reshape(-1).contiguous()
                if yp.numel() != yy.numel() or yp.numel() % batch:
                    raise ValueError("y and y_pred must hold the same number of elements, a multiple of the number of segment ids")
                self.per_window = yp.numel() // batch
                eng._check(self.lib, self.lib.mshgnn_metrics_regression_segmented(yp.data_ptr(), yy.data_ptr(), batch, self.per_window, seg.data_ptr(), self.n_segments,
                                                                                  self.state.data_ptr(), self._scratch.data_ptr(), _stream(dev)),
                           "mshgnn_metrics_regression_segmented")
            else:
                if y_pred.numel() != batch * 8 or y.numel() != batch * 4:
                    raise ValueError("expected logits [batch * 4, 2] and labels [batch, 4] for the segment ids given")
                yp = y_pred.detach().to(dev, torch.float32).reshape(batch * 4, 2).contiguous()
                yy = y.detach().to(dev, torch.int32).reshape(batch * 4).contiguous()
                eng._check(self.lib, self.lib.mshgnn_metrics_classification_segmented(yp.data_ptr(), yy.data_ptr(), batch, seg.data_ptr(), self.n_segments,
                                                                                      self.state.data_ptr(), self.counts.data_ptr(), self._scratch.data_ptr(),
                                                                                      _stream(dev)),
                           "mshgnn_metrics_classification_segmented")

    def table(self) -> dict:
        """fp64 device tensors [n_segments] (`table_from_state`); no synchronisation."""
        n = self.n_segments
        return table_from_state(self.state[:n], None if self.regression else self.counts[:n], self.per_window)

    def overflow(self) -> int:
        """Windows whose id was outside [0, n_segments) since the last reset (one host synchronisation)."""
        if self.regression:
            return int(round(float(self.state[self.n_segments, 2].item()) / self.per_window))
        return int(self.counts[self.n_segments, 0].item())

    def check(self) -> None:
        n = self.overflow()
        if n:
            raise IndexError(f"{n} windows carried a segment id outside [0, {self.n_segments})")

    def reset(self) -> None:
        self.state.zero_()
        if self.counts is not None:
            self.counts.zero_()


class SegmentedComMetrics:
    """The sums of `ComStepMetrics` per segment (mshgnn_metrics_com_segmented, include/mshgnn.h): `update(y, y_pred, segment)` adds every window's squared
    errors of the lin / ang halves and the two cosines of base node 0 to the row its id names, in ONE launch, bit-reproducibly (no floating-point
    atomic).  The interface of `SegmentedMetrics`; `state` is fp64 [n_segments + 1][8] in the layout of mshgnn_metrics_com_step, the last row the overflow row."""

    def __init__(self, n_segments: int, num_bases: int, y_mean, y_std, device=None):
        if int(n_segments) < 1 or int(num_bases) < 1:
            raise ValueError("n_segments and num_bases must be >= 1")
        self.n_segments, self.num_bases = int(n_segments), int(num_bases)
        mean = [float(v) for v in torch.as_tensor(y_mean, dtype=torch.float64).flatten().tolist()]
        std = [float(v) for v in torch.as_tensor(y_std, dtype=torch.float64).flatten().tolist()]
        if len(mean) != 6 or len(std) != 6:
            raise ValueError("y_mean and y_std must have 6 entries (lin(3) | ang(3))")
        self._mean, self._std = (C.c_double * 6)(*mean), (C.c_double * 6)(*std)
        self.device = _device(device)
        self.lib = eng.load_library()
        if not hasattr(self.lib, "mshgnn_metrics_com_segmented"):
            raise eng.MshgnnError("this build of the library has no mshgnn_metrics_com_segmented")
        self.state = torch.zeros(self.n_segments + 1, 8, dtype=torch.float64, device=self.device)
        self._scratch, self._scratch_batch = None, 0

    def reserve(self, batch: int) -> None:
        """The scratch for batches of up to `batch` windows (`update` grows it when needed; reserve before capturing `update` in a graph)."""
        if batch > self._scratch_batch:
            nbytes = int(self.lib.mshgnn_metrics_com_segmented_scratch_bytes(int(batch)))
            self._scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=self.device)      # zeroed once; the calls own it from here
            self._scratch_batch = int(batch)

    def update(self, y: torch.Tensor, y_pred: torch.Tensor, segment: torch.Tensor) -> None:
        """y / y_pred: batch x num_bases x 6 values as `ComStepMetrics.calculate_losses_step` takes them, segment: int32 [batch] on the device."""
        dev = self.device
        seg = segment.detach().to(dev, torch.int32).reshape(-1).contiguous()
        batch = int(seg.numel())
        if batch < 1:
            raise ValueError("no windows")
        yp = y_pred.detach().to(dev, torch.float32).reshape(-1).contiguous()
        yy = y.detach().to(dev, torch.float32).reshape(-1).contiguous()
        if yp.numel() != yy.numel() or yp.numel() != batch * self.num_bases * 6:
            raise ValueError(f"y and y_pred must hold {self.num_bases} x 6 values for each of the {batch} segment ids")
        self.reserve(batch)
        with torch.cuda.device(dev):
            eng._check(self.lib, self.lib.mshgnn_metrics_com_segmented(yp.data_ptr(), yy.data_ptr(), batch, self.num_bases, self._mean, self._std, seg.data_ptr(),
                                                                       self.n_segments, self.state.data_ptr(), self._scratch.data_ptr(), _stream(dev)),
                       "mshgnn_metrics_com_segmented")

    def table(self) -> dict:
        """fp64 device tensors [n_segments] (`com_table_from_state`); no synchronisation."""
        return com_table_from_state(self.state[:self.n_segments])

    def overflow(self) -> int:
        """Windows whose id was outside [0, n_segments) since the last reset (one host synchronisation)."""
        return int(round(float(self.state[self.n_segments, 6].item())))

    def check(self) -> None:
        n = self.overflow()
        if n:
            raise IndexError(f"{n} windows carried a segment id outside [0, {self.n_segments})")

    def reset(self) -> None:
        self.state.zero_()
