"""The training-step wrappers around the MS-HGNN models: host-side mirror of the reference's Lightning modules for the hot path.

Same class names, constructor arguments, method names and return values as `src/ms_hgnn/lightning_py/gnnLightning.py`:
`Base_Lightning` (:28-348), `Heterogeneous_GNN_Lightning` (:415-462), `HGNN_K4_Lightning` (:464-513), `HGNN_C2_Lightning_Cls`
(:515-562), `HGNN_C2_Lightning_Reg` (:564-778), and of `gnnLightning_com.py`: `COM_Base_Lightning` (:28-232), `COM_HGNN_Lightning`
(:290-340), `COM_HGNN_SYM_Lightning` (:343-409).  What differs is where the work runs: the model is this package's (HIP engine), the
metric bookkeeping is `metrics.StepMetrics` (one launch per step, the returned loss carries autograd) and the world-frame rotation of
the GRFs stays on the device instead of the reference's per-step CPU + scipy hop (:663-676).

`lightning` is not a dependency: with it installed the wrappers ARE `LightningModule`s and a `Trainer` drives them unchanged; without
it they are plain `nn.Module`s whose `log()` records the values in `self.logged`, and `examples/` / `tests/` drive the same methods
(`training_step`, `validation_step`, `on_validation_epoch_end`, `configure_optimizers`) by hand.  Datasets, checkpoint callbacks, W&B
logging and `train_model` / `evaluate_model` are out of scope (control plane).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import nn, optim

from . import models
from .metrics import StepMetrics

try:  # pragma: no cover - lightning is absent in the build image
    import lightning as _L
    _Base = _L.LightningModule
except Exception:  # noqa: BLE001
    _L = None
    _Base = nn.Module

_REG = ("MSE_loss", "mse_loss"), ("RMSE_loss", "rmse_loss"), ("L1_loss", "l1_loss")
_METRIC_ATTRS = ("mse_loss", "rmse_loss", "l1_loss", "ce_loss", "acc", "f1_leg0", "f1_leg1", "f1_leg2", "f1_leg3")


def _metric_property(name):
    def get(self):
        m = self.__dict__.get("_metrics")
        return None if m is None or name not in m._names() else getattr(m, name)
    return property(get)


def _model_fused_step(wrapper, batch):
    """(out, loss) from the model's one-call training step -- for a `windows.WindowBatch` with the window gather fused into the encoder --
    or None when the wrapper has to take the two-call route."""
    if not wrapper.fused_training_step:
        return None
    from .windows import WindowBatch
    if isinstance(batch, WindowBatch):
        r = wrapper.model.fused_training_step_windows(batch)
        if r is not None:
            return r
    return wrapper.model.fused_training_step(batch.x_dict, batch.edge_index_dict, batch.y)


def _model_forward(wrapper, batch):
    """The model's output for a batch: for a `windows.WindowBatch` without autograd (validation, test, prediction) straight from the sequence's resident
    series (models.forward_windows -- no assembled windows; the labels are left on the batch), else -- or where that route does not apply, or with
    `fused_evaluation_step = False` -- the model's own forward over `batch.x_dict`.  Same bits either way."""
    if wrapper.fused_evaluation_step and not torch.is_grad_enabled():
        from .windows import WindowBatch
        if isinstance(batch, WindowBatch) and hasattr(wrapper.model, "forward_windows"):
            out = wrapper.model.forward_windows(batch)
            if out is not None:
                return out
    return wrapper.model(x_dict=batch.x_dict, edge_index_dict=batch.edge_index_dict)


def _at_f64(wrapper) -> bool:
    """The wrapper's model runs at precision "f64" (models.set_precision): fp64 parameters, fp64 operators, no fused engine."""
    return getattr(getattr(wrapper, "model", None), "_precision", None) == "f64"


def _f64_step_loss(regression: bool, y: torch.Tensor, y_pred: torch.Tensor, reg_loss=("mse", 1.0)) -> torch.Tensor:
    """The step loss of an "f64" model in fp64 torch operations on [batch, out] (the GEMMs are the hot path, not this): the MSE over every element -- with
    `reg_loss` ("l1", _) / ("huber", delta) the mean L1 / Huber loss (set_regression_loss) --, or the
    mean cross entropy of the per-foot [stable, contact] logits against the contact flags (y != 0) -- what the metric kernels compute in fp32.  Carries
    autograd to y_pred; an fp64 tensor with an fp64 gradient."""
    yp = y_pred.to(torch.float64)
    if regression:
        yy = y.detach().to(yp.device, torch.float64).reshape(yp.shape)
        if reg_loss[0] == "l1":
            return torch.nn.functional.l1_loss(yp, yy)
        if reg_loss[0] == "huber":
            return torch.nn.functional.huber_loss(yp, yy, delta=float(reg_loss[1]))
        return torch.mean((yp - yy) ** 2)
    logits = yp.reshape(-1, 2)
    return torch.nn.functional.cross_entropy(logits, (y.detach().to(yp.device) != 0).to(torch.long).reshape(-1))


def _reg_loss_of(wrapper):
    """(kind, delta) of the wrapper's training loss: the MODEL's (models.set_regression_loss), the one place it is kept -- so `model.set_regression_loss`, the
    wrapper's own and a `Symmetrised` view's (same model) all mean the same thing to every wrapper over that model."""
    return getattr(getattr(wrapper, "model", None), "regression_loss", ("mse", 1.0))


def _set_regression_loss(wrapper, kind: str, delta: float = 1.0):
    """`set_regression_loss` of every regression wrapper: the model's (its fused engines, or the kind kept for "f64"); the step metrics follow per step (`_synced`)."""
    wrapper.model.set_regression_loss(kind, delta)      # (ValueError on a classification model, a bad kind or delta)
    return wrapper


def _synced(wrapper, metrics):
    """The wrapper's step metrics told the model's kind (every `_m()`: each step passes here before it publishes anything)."""
    if metrics.regression and metrics.reg_loss != _reg_loss_of(wrapper) and getattr(wrapper, "regression", True):
        metrics.set_regression_loss(*_reg_loss_of(wrapper))
    return metrics


def _robust(wrapper) -> bool:
    return wrapper.regression and _reg_loss_of(wrapper)[0] != "mse"


def _losses_step(wrapper, y, y_pred):
    """calculate_losses_step of every wrapper.  A model at "f64": the published / returned loss is `_f64_step_loss` (it never passes the fp32 loss kernel),
    while the LOGGED metric values (rmse, l1, accuracy, F1, the epoch sums) keep coming from the metric kernels on an fp32 copy of the predictions."""
    if _at_f64(wrapper) and torch.is_grad_enabled() and y_pred.requires_grad:
        wrapper._m().calculate_losses_step(y, y_pred.detach())
        wrapper._m().set_step_loss(_f64_step_loss(wrapper.regression, y, y_pred, _reg_loss_of(wrapper)))
    elif _at_f64(wrapper):
        wrapper._m().calculate_losses_step(y, y_pred)
        with torch.no_grad():
            wrapper._m().set_step_loss(_f64_step_loss(wrapper.regression, y, y_pred, _reg_loss_of(wrapper)))
    else:
        wrapper._m().calculate_losses_step(y, y_pred)


class Base_Lightning(_Base):
    """Steps, epoch hooks, logging and the optimizer shared by every wrapper (gnnLightning.py:28-348)."""

    # training_step hands the labels to the model, which runs forward + loss + backward as ONE engine call (models.fused_training_step:
    # the decoder, the loss and the decoder's backward sit in the tail of the fused forward kernel); the returned loss delivers those
    # gradients when backward() is called on it.  Same loss and gradients as the two-call route, which is taken when this is False
    # (an attribute, set per wrapper or on the class), under torch.distributed, with host parameters, or without autograd.
    fused_training_step = True
    # validation_step / test_step / predict_step on a windows.WindowBatch under torch.no_grad(): the engine's encoder gathers the windows from the resident
    # series (models.forward_windows, mshgnn_forward_series) instead of reading assembled ones; False: always assemble, then forward.  Same bits.
    fused_evaluation_step = True
    # configure_optimizers hands these to the flat optimizers (optim.py): the step count / the learning rate live on the device, so that the step can be
    # captured in a HIP graph (GraphedTrainingStep) and a captured step follows a learning-rate scheduler.
    graph_safe_optimizer = False
    device_lr_optimizer = False

    def __init__(self, optimizer: str, lr: float, regression: bool):
        super().__init__()
        self.optimizer = optimizer
        self.lr = lr
        self.regression = regression
        self.body_to_world_frame = False
        self.__dict__["_metrics"] = None            # metrics.StepMetrics, created with the first step (it needs the device)
        self.__dict__["_metrics_world"] = None
        self.logged = {}

    # ---- metric state ------------------------------------------------------------------------------------------------
    def _m(self, world: bool = False) -> StepMetrics:
        key = "_metrics_world" if world else "_metrics"
        if self.__dict__[key] is None:
            self.__dict__[key] = StepMetrics(regression=True if world else self.regression)
        return self.__dict__[key] if world else _synced(self, self.__dict__[key])

    def set_regression_loss(self, kind: str, delta: float = 1.0):
        """Train on "mse" (the default, the reference's), "l1" or "huber" with `delta` (torch.nn.L1Loss / HuberLoss(delta)): `training_step` returns that loss on
        the fused and on the two-call route and logs it as "train_loss" next to the metric values, which stay what they are (`mse_loss`, `rmse_loss`, `l1_loss`);
        `validation_step` / `test_step` keep returning `mse_loss`.  ValueError on a classification wrapper."""
        return _set_regression_loss(self, kind, delta)

    loss = property(lambda self: None if self.__dict__.get("_metrics") is None else self.__dict__["_metrics"].loss)

    if _L is None:
        def log(self, name, value, on_step: bool = False, on_epoch: bool = True, **_):
            """Stand-in for LightningModule.log: the last value per name (a device tensor; reading it is the caller's sync)."""
            self.logged[name] = value

    def log_losses(self, step_name: str, on_step: bool):
        on_epoch = not on_step
        if self.regression:
            for label, attr in _REG:
                self.log(f"{step_name}_{label}", getattr(self, attr), on_step=on_step, on_epoch=on_epoch)
            if _robust(self) and on_step:      # the L1 / Huber training loss of the step (no epoch value: validation and test report the metrics)
                self.log(f"{step_name}_loss", self.loss, on_step=on_step, on_epoch=on_epoch)
        else:
            self.log(step_name + "_CE_loss", self.ce_loss, on_step=on_step, on_epoch=on_epoch)
            self.log(step_name + "_Accuracy", self.acc, on_step=on_step, on_epoch=on_epoch)
            f1 = [self.f1_leg0, self.f1_leg1, self.f1_leg2, self.f1_leg3]
            self.log(step_name + "_F1_Score_Leg_Avg", (f1[0] + f1[1] + f1[2] + f1[3]) / 4.0, on_step=on_step, on_epoch=on_epoch)
            for k in range(4):
                self.log(f"{step_name}_F1_Score_Leg_{k}", f1[k], on_step=on_step, on_epoch=on_epoch)

    def calculate_losses_step(self, y: torch.Tensor, y_pred: torch.Tensor):
        """gnnLightning.py:124-151.  Classification: `y_pred` [batch, 8] logits, `y` [batch, 4] contact flags.  A model at precision "f64": the loss is
        computed in fp64 (`_losses_step`); the other logged values come from the fp32 metric kernels."""
        _losses_step(self, y, y_pred)

    def calculate_losses_epoch(self) -> None:
        self._m().calculate_losses_epoch()

    def reset_all_metrics(self) -> None:
        self._m().reset_all_metrics()

    def _loss(self):
        return self.mse_loss if self.regression else self.ce_loss

    def _train_loss(self):
        return self.loss if _robust(self) else self._loss()

    # ---- steps (gnnLightning.py:179-256) -----------------------------------------------------------------------------
    def training_step(self, batch, batch_idx):
        y, y_pred = self.step_helper_function(batch)
        self.calculate_losses_step(y, y_pred)
        self.log_losses("train", on_step=True)
        return self._train_loss()

    def on_validation_epoch_start(self):
        self.reset_all_metrics()

    def validation_step(self, batch, batch_idx):
        y, y_pred = self.step_helper_function(batch)
        self.calculate_losses_step(y, y_pred)
        return self._loss()

    def on_validation_epoch_end(self):
        self.calculate_losses_epoch()
        self.log_losses("val", on_step=False)

    def on_test_epoch_start(self):
        self.reset_all_metrics()

    def test_step(self, batch, batch_idx):
        return self.validation_step(batch, batch_idx)

    def on_test_epoch_end(self):
        self.calculate_losses_epoch()
        self.log_losses("test", on_step=False)

    def on_predict_start(self):
        self.reset_all_metrics()

    def predict_step(self, batch, batch_idx):
        y, y_pred = self.step_helper_function(batch)
        self.calculate_losses_step(y, y_pred)
        if not self.regression:
            raise NotImplementedError("This prediction method is not fully tested for classification.")
        return y, y_pred

    def on_predict_end(self):
        self.calculate_losses_epoch()

    # ---- optimizer (gnnLightning.py:258-265) -------------------------------------------------------------------------
    def configure_optimizers(self):
        model = getattr(self, "model", None)
        flat = isinstance(model, models._MSHGNNBase) and len(list(self.parameters())) == len(list(model.parameters()))
        flat = flat and not _at_f64(self)      # (the flat optimizers step fp32 flat buffers; an "f64" model's fp64 parameters get torch's own optimizer)
        on_device = dict(graph_safe=bool(getattr(self, "graph_safe_optimizer", False)),      # (graph_safe: GraphedTrainingStep)
                         device_lr=bool(getattr(self, "device_lr_optimizer", False)))      # (device_lr: a captured step follows a scheduler)
        if self.optimizer == "adam":
            if flat:
                from .optim import FlatAdam      # a torch.optim.Adam whose step is one launch on the flat buffers (torch's own step otherwise)
                return FlatAdam(model, lr=self.lr, **on_device)
            return optim.Adam(self.parameters(), lr=self.lr)
        if self.optimizer == "sgd":
            if flat:
                from .optim import FlatSGD      # the same for torch.optim.SGD
                return FlatSGD(model, lr=self.lr, **on_device)
            return optim.SGD(self.parameters(), lr=self.lr)
        raise ValueError("Invalid optimizer setting")

    # ---- helpers -----------------------------------------------------------------------------------------------------
    def step_helper_function(self, batch):
        raise NotImplementedError

    def classification_calculate_useful_values(self, y_pred, batch_size):
        """Per-foot logits [batch*4, 2], their softmax, and the contact probabilities [batch, 4] (gnnLightning.py:285-304)."""
        per_foot = torch.reshape(y_pred, (batch_size * 4, 2))
        prob = torch.nn.functional.softmax(per_foot, dim=1)
        return per_foot, prob, torch.reshape(prob[:, 1], (batch_size, 4))

    @staticmethod
    def classification_conversion_16_class(y_pred_per_foot_prob_only_1: torch.Tensor, y: torch.Tensor):
        return StepMetrics.classification_conversion_16_class(y_pred_per_foot_prob_only_1, y)


for _n in _METRIC_ATTRS:
    setattr(Base_Lightning, _n, _metric_property(_n))


class _HGNNWrapper(Base_Lightning):
    """What the four GRF wrappers share: build the model, run the lazy-initialising dummy forward (:445-447), reshape outputs and labels
    per window (:449-462, :495-513, :680-695)."""

    _label_width_is_output_width = False      # y: [batch, out_channels_per_foot * 4] (True) or [batch, 4] (False)

    def _finish_init(self, dummy_batch):
        with torch.no_grad():
            self.model(x_dict=dummy_batch.x_dict, edge_index_dict=dummy_batch.edge_index_dict)
        if _L is not None:  # pragma: no cover
            self.save_hyperparameters(ignore=["dummy_batch", "activation_fn"])

    def _shape(self, batch, out_raw):
        batch_size = batch.batch_size if hasattr(batch, "batch_size") else 1
        width = self.model.out_channels_per_foot * 4
        y_pred = torch.reshape(out_raw.squeeze(), (batch_size, width))
        y = torch.reshape(batch.y, (batch_size, width if self._label_width_is_output_width else 4))
        return y, y_pred

    def step_helper_function(self, batch):
        return self._shape(batch, _model_forward(self, batch))

    def _fused_step(self, batch):
        """(y, y_pred, loss) from the one-call engine step, or None when that route does not apply."""
        r = _model_fused_step(self, batch)
        if r is None:
            return None
        y, y_pred = self._shape(batch, r[0])
        return y, y_pred, r[1]

    def training_step(self, batch, batch_idx):
        r = self._fused_step(batch)
        if r is None:
            return super().training_step(batch, batch_idx)
        y, y_pred, loss = r
        self.calculate_losses_step(y, y_pred)          # the step's metric sums (y_pred carries no autograd here)
        self._m().set_step_loss(loss)
        self.log_losses("train", on_step=True)
        return loss


class Heterogeneous_GNN_Lightning(_HGNNWrapper):
    """MI-HGNN baseline `GRF_HGNN` (gnnLightning.py:415-462)."""
    _label_width_is_output_width = True

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), grf_dimension: int = 1):
        super().__init__(optimizer, lr, regression)
        self.model = models.GRF_HGNN(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata,
                                     regression=regression, activation_fn=activation_fn, grf_dimension=grf_dimension)
        self._finish_init(dummy_batch)


class HGNN_K4_Lightning(_HGNNWrapper):
    """`GRF_HGNN_K4` (gnnLightning.py:464-513): labels [batch, 4] (1-D GRFs or contact flags)."""

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), symmetry_mode: Optional[str] = None,
                 group_operator_path: Optional[str] = None):
        super().__init__(optimizer, lr, regression)
        self.model = models.GRF_HGNN_K4(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata,
                                        regression=regression, activation_fn=activation_fn, symmetry_mode=symmetry_mode,
                                        group_operator_path=group_operator_path)
        self._finish_init(dummy_batch)


class HGNN_C2_Lightning_Cls(_HGNNWrapper):
    """`GRF_HGNN_C2` for contact classification (gnnLightning.py:515-562)."""

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), symmetry_mode: Optional[str] = None,
                 group_operator_path: Optional[str] = None):
        super().__init__(optimizer, lr, regression)
        self.model = models.GRF_HGNN_C2(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata,
                                        regression=regression, activation_fn=activation_fn, symmetry_mode=symmetry_mode,
                                        group_operator_path=group_operator_path)
        self._finish_init(dummy_batch)


class HGNN_C2_Lightning_Reg(_HGNNWrapper):
    """`GRF_HGNN_C2` for GRF regression, optionally with the metrics ALSO evaluated in the world frame (gnnLightning.py:564-778): with
    `grf_body_to_world_frame` the labels / predictions are rotated by the inverse of `batch.r_o` (world->body quaternions, scalar last)
    on the device and a second metric state accumulates them; the loss that is returned stays the body-frame MSE (:709-716)."""
    _label_width_is_output_width = True

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), symmetry_mode: Optional[str] = None,
                 group_operator_path: Optional[str] = None, grf_body_to_world_frame: Optional[bool] = None, grf_dimension: int = 3):
        super().__init__(optimizer, lr, regression)
        self.model = models.GRF_HGNN_C2(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata,
                                        regression=regression, activation_fn=activation_fn, symmetry_mode=symmetry_mode,
                                        group_operator_path=group_operator_path, grf_dimension=grf_dimension)
        self._finish_init(dummy_batch)
        self.body_to_world_frame = bool(grf_body_to_world_frame) if regression else False

    # world-frame values: read from the second metric state
    mse_loss_worldframe = property(lambda self: None if self.__dict__["_metrics_world"] is None else self._m(True).mse_loss)
    rmse_loss_worldframe = property(lambda self: None if self.__dict__["_metrics_world"] is None else self._m(True).rmse_loss)
    l1_loss_worldframe = property(lambda self: None if self.__dict__["_metrics_world"] is None else self._m(True).l1_loss)

    def body_frame_to_world_frame(self, batch_r_quat, grf_bodyFrame):
        return self._m().body_frame_to_world_frame(batch_r_quat, grf_bodyFrame)

    def calculate_losses_step_original(self, y: torch.Tensor, y_pred: torch.Tensor):
        Base_Lightning.calculate_losses_step(self, y, y_pred)

    def calculate_losses_step_worldframe(self, y, y_pred, batch_r_quat, test_only_on_z: bool = False):
        self.calculate_losses_step_original(y, y_pred)
        y_world = self.body_frame_to_world_frame(batch_r_quat, y.detach())
        y_pred_world = self.body_frame_to_world_frame(batch_r_quat, y_pred.detach())
        if test_only_on_z:
            y_world, y_pred_world = y_world[:, [2, 5, 8, 11]], y_pred_world[:, [2, 5, 8, 11]]
        self._m(True).calculate_losses_step(y_world, y_pred_world)

    def calculate_losses_step(self, y, y_pred, batch_r_quat=None):
        if self.body_to_world_frame:
            if batch_r_quat is None:
                raise ValueError("grf_body_to_world_frame needs the batch's r_o quaternions")
            self.calculate_losses_step_worldframe(y, y_pred, batch_r_quat)
        else:
            self.calculate_losses_step_original(y, y_pred)

    def log_losses_worldframe(self, step_name: str, on_step: bool):
        self.log_losses(step_name, on_step)
        for label, attr in _REG:
            self.log(f"{step_name}_{label}_WorldFrame", getattr(self, attr + "_worldframe"), on_step=on_step, on_epoch=not on_step)

    def calculate_losses_epoch_worldframe(self) -> None:
        self.calculate_losses_epoch()
        self._m(True).calculate_losses_epoch()

    def reset_all_metrics_worldframe(self) -> None:
        self.reset_all_metrics()
        self._m(True).reset_all_metrics()

    def _step(self, batch):
        y, y_pred = self.step_helper_function(batch)
        if self.body_to_world_frame:
            self.calculate_losses_step_worldframe(y, y_pred, batch.r_o.view(batch.batch_size, 4))
        else:
            self.calculate_losses_step_original(y, y_pred)

    def training_step(self, batch, batch_idx):
        r = self._fused_step(batch)
        if r is None:
            self._step(batch)
        else:
            y, y_pred, loss = r
            if self.body_to_world_frame:
                self.calculate_losses_step_worldframe(y, y_pred, batch.r_o.view(batch.batch_size, 4))
            else:
                self.calculate_losses_step_original(y, y_pred)
            self._m().set_step_loss(loss)
        (self.log_losses_worldframe if self.body_to_world_frame else self.log_losses)("train", on_step=True)
        return self._train_loss()

    def validation_step(self, batch, batch_idx):
        self._step(batch)
        return self._loss()

    def on_validation_epoch_start(self):
        (self.reset_all_metrics_worldframe if self.body_to_world_frame else self.reset_all_metrics)()

    def on_validation_epoch_end(self):
        if self.body_to_world_frame:
            self.calculate_losses_epoch_worldframe()
            self.log_losses_worldframe("val", on_step=False)
        else:
            self.calculate_losses_epoch()
            self.log_losses("val", on_step=False)

    def on_test_epoch_start(self):
        self.on_validation_epoch_start()

    def on_test_epoch_end(self):
        if self.body_to_world_frame:
            self.calculate_losses_epoch_worldframe()
            self.log_losses_worldframe("test", on_step=False)
        else:
            self.calculate_losses_epoch()
            self.log_losses("test", on_step=False)


# ---- centroidal-momentum wrappers (src/ms_hgnn/lightning_py/gnnLightning_com.py) ---------------------------------------------------
_COM_LOGS = (("MSE_loss", "mse_loss"), ("RMSE_loss", "rmse_loss"), ("MSE_loss_lin", "mse_loss_lin"), ("MSE_loss_ang", "mse_loss_ang"),
             ("cos_sim_lin", "cos_sim_lin"), ("cos_sim_ang", "cos_sim_ang"), ("avg_cos_sim", "avg_cos_sim"), ("loss", "loss"))


class COM_Base_Lightning(_Base):
    """`COM_Base_Lightning` (gnnLightning_com.py:28-232).  `data_path` is the dataset folder whose `processed/rss_stats.npz` holds the
    label statistics (`y_mean`, `y_std`) the cosine-similarity metrics un-standardise with (:52-58); `stats=(y_mean, y_std)` hands them
    over directly (synthetic data, tests)."""

    def __init__(self, optimizer: str, lr: float, data_path=None, stats=None):
        super().__init__()
        self.optimizer, self.lr, self.data_path = optimizer, lr, data_path
        self.regression = True
        if stats is None:
            import os
            import numpy as np
            if data_path is None:
                raise ValueError("COM wrappers need data_path (processed/rss_stats.npz) or stats=(y_mean, y_std)")
            st = np.load(os.path.join(str(data_path), "processed", "rss_stats.npz"))
            stats = (st["y_mean"], st["y_std"])
        self.__dict__["_stats"] = stats
        self.__dict__["_metrics"] = None
        self.logged = {}

    def _m(self):
        if self.__dict__["_metrics"] is None:
            from .metrics import ComStepMetrics
            self.__dict__["_metrics"] = ComStepMetrics(self.model.num_bases, *self.__dict__["_stats"])
        return _synced(self, self.__dict__["_metrics"])

    def set_regression_loss(self, kind: str, delta: float = 1.0):
        """Base_Lightning.set_regression_loss for the centroidal-momentum wrappers: `loss` (what training_step returns and logs) becomes the L1 / Huber loss."""
        return _set_regression_loss(self, kind, delta)

    if _L is None:
        def log(self, name, value, on_step: bool = False, on_epoch: bool = True, **_):
            self.logged[name] = value

    def log_losses(self, step_name: str, on_step: bool):
        for label, attr in _COM_LOGS:
            self.log(f"{step_name}_{label}", getattr(self, attr), on_step=on_step, on_epoch=not on_step)

    def calculate_losses_step(self, y: torch.Tensor, y_pred: torch.Tensor):
        _losses_step(self, y, y_pred)

    def calculate_losses_epoch(self) -> None:
        self._m().calculate_losses_epoch()

    def reset_all_metrics(self) -> None:
        self._m().reset_all_metrics()

    fused_training_step = Base_Lightning.fused_training_step
    fused_evaluation_step = Base_Lightning.fused_evaluation_step

    def training_step(self, batch, batch_idx):
        r = _model_fused_step(self, batch)
        if r is None:
            y, y_pred = self.step_helper_function(batch)
            self.calculate_losses_step(y, y_pred)
        else:
            y, y_pred = self._shape(batch, r[0])
            self.calculate_losses_step(y, y_pred)
            self._m().set_step_loss(r[1])
        self.log_losses("train", on_step=True)
        return self.loss

    def on_validation_epoch_start(self):
        self.reset_all_metrics()

    def validation_step(self, batch, batch_idx):
        y, y_pred = self.step_helper_function(batch)
        self.calculate_losses_step(y, y_pred)
        return self.mse_loss if _robust(self) else self.loss      # (validation and test report the MSE at every training loss, as the reference does)

    def on_validation_epoch_end(self):
        self.calculate_losses_epoch()
        self.log_losses("val", on_step=False)

    def on_test_epoch_start(self):
        self.reset_all_metrics()

    def test_step(self, batch, batch_idx):
        return self.validation_step(batch, batch_idx)

    def on_test_epoch_end(self):
        self.calculate_losses_epoch()
        self.log_losses("test", on_step=False)

    def configure_optimizers(self):
        return Base_Lightning.configure_optimizers(self)

    def step_helper_function(self, batch):
        """Outputs and labels per window, [batch, num_bases * 6] (gnnLightning_com.py:324-340, 394-409)."""
        return self._shape(batch, _model_forward(self, batch))

    def _shape(self, batch, out_raw):
        batch_size = batch.batch_size if hasattr(batch, "batch_size") else 1
        width = self.model.num_bases * self.model.num_dimensions_per_base
        return torch.reshape(batch.y, (batch_size, width)), torch.reshape(out_raw.squeeze(), (batch_size, width))

    def _finish_init(self, dummy_batch):
        with torch.no_grad():
            self.model(x_dict=dummy_batch.x_dict, edge_index_dict=dummy_batch.edge_index_dict)
        if _L is not None:  # pragma: no cover
            self.save_hyperparameters(ignore=["dummy_batch", "activation_fn"])


for _n in ("mse_loss", "rmse_loss", "mse_loss_lin", "mse_loss_ang", "cos_sim_lin", "cos_sim_ang", "avg_cos_sim", "loss"):
    setattr(COM_Base_Lightning, _n, property(lambda self, _n=_n: None if self.__dict__.get("_metrics") is None else getattr(self.__dict__["_metrics"], _n)))


class COM_HGNN_Lightning(COM_Base_Lightning):
    """`COM_HGNN` (one base node, no symmetry; gnnLightning_com.py:290-340)."""

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), com_dimension: int = 6, data_path=None, stats=None):
        super().__init__(optimizer, lr, data_path, stats)
        self.model = models.COM_HGNN(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata, regression=regression,
                                     activation_fn=activation_fn, com_dimension=com_dimension)
        self.regression = regression
        self._finish_init(dummy_batch)


class COM_HGNN_SYM_Lightning(COM_Base_Lightning):
    """`COM_HGNN_K4` / `COM_HGNN_C2` / `COM_HGNN_S4` by `model_type` (gnnLightning_com.py:343-409)."""

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, dummy_batch, optimizer: str = "adam", lr: float = 0.003,
                 regression: bool = True, activation_fn=nn.ReLU(), symmetry_mode: Optional[str] = None, group_operator_path: Optional[str] = None,
                 model_type: str = "heterogeneous_gnn_k4_com", data_path=None, stats=None):
        super().__init__(optimizer, lr, data_path, stats)
        common = dict(hidden_channels=hidden_channels, num_layers=num_layers, data_metadata=data_metadata, regression=regression,
                      activation_fn=activation_fn)
        if model_type == "heterogeneous_gnn_k4_com":
            self.model = models.COM_HGNN_K4(symmetry_mode=symmetry_mode, group_operator_path=group_operator_path, **common)
        elif model_type == "heterogeneous_gnn_c2_com":
            self.model = models.COM_HGNN_C2(symmetry_mode=symmetry_mode, group_operator_path=group_operator_path, **common)
        elif model_type == "heterogeneous_gnn_s4_com":
            self.model = models.COM_HGNN_S4(**common)
        else:
            raise ValueError(f"unknown model_type '{model_type}'")
        self.regression = regression
        self._finish_init(dummy_batch)


class _MLPSteps:
    """What the two MLP wrappers share: `step_helper_function` for a `windows.WindowBatch` of an `windows.mlp_recipe` store (under no_grad: straight from the
    resident series, MLPEngine.forward_series) or the reference's `(x, y)` tuple batch, and the one-call training step (MLPEngine.step_*_series / step_*)."""

    def _rows(self, batch):
        from .windows import WindowBatch
        if isinstance(batch, WindowBatch):
            t = batch.store.recipe.node_types[0]
            return batch.x_dict[t][:, :self.model.in_channels], batch.y
        x, y = batch
        return x, y

    def step_helper_function(self, batch):
        from .windows import WindowBatch
        m = self.model
        if isinstance(batch, WindowBatch) and self.fused_evaluation_step and not torch.is_grad_enabled():
            out = m.forward_windows(batch)
            if out is not None:
                return batch.y, out
        x, y = self._rows(batch)
        return y, m(x)

    def _fused_mlp_step(self, batch):
        """(y, y_pred, loss) from the one-call step, or None when the two-call route has to be taken."""
        if not self.fused_training_step:
            return None
        from .windows import WindowBatch
        m = self.model
        if isinstance(batch, WindowBatch):
            r = m.fused_training_step_windows(batch)
            if r is not None:
                return batch.y, r[0], r[1]
        x, y = self._rows(batch)
        r = m.fused_training_step(x, y)
        return None if r is None else (y, r[0], r[1])


class MLP_Lightning(_MLPSteps, Base_Lightning):
    """`MLP_Lightning` (gnnLightning.py:363-413): the MLP baseline every table of the paper compares against.  `mlp_model` is a `models.MLP` with the
    reference's parameter names (`mlp_model.0.weight`, ...); `model` is the same module."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int, batch_size: int, optimizer: str = "adam",
                 lr: float = 0.003, regression: bool = True, activation_fn=nn.ReLU()):
        super().__init__(optimizer, lr, regression)
        self.batch_size = batch_size
        self.regression = regression
        self.mlp_model = models.MLP(in_channels, hidden_channels, out_channels, num_layers, activation_fn, regression=regression)
        if _L is not None:  # pragma: no cover
            self.save_hyperparameters(ignore=["activation_fn"])

    model = property(lambda self: self.mlp_model)

    def training_step(self, batch, batch_idx):
        r = self._fused_mlp_step(batch)
        if r is None:
            return Base_Lightning.training_step(self, batch, batch_idx)
        y, y_pred, loss = r
        self.calculate_losses_step(y, y_pred)
        self._m().set_step_loss(loss)
        self.log_losses("train", on_step=True)
        return loss


class COM_MLP_Lightning(_MLPSteps, COM_Base_Lightning):
    """`COM_MLP_Lightning` (gnnLightning_com.py:234-287): the MLP baseline of the centroidal-momentum task; `model.num_bases = 1`,
    `model.num_dimensions_per_base = 6`."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int, batch_size: int, optimizer: str = "adam",
                 lr: float = 0.003, regression: bool = True, activation_fn=nn.ReLU(), data_path=None, stats=None):
        super().__init__(optimizer, lr, data_path, stats)
        self.batch_size = batch_size
        self.regression = regression
        self.model = models.MLP(in_channels, hidden_channels, out_channels, num_layers, activation_fn, regression=True)
        self.model.num_bases = 1
        self.model.num_dimensions_per_base = 6
        if _L is not None:  # pragma: no cover
            self.save_hyperparameters(ignore=["activation_fn"])

    def training_step(self, batch, batch_idx):
        r = self._fused_mlp_step(batch)
        if r is None:
            y, y_pred = self.step_helper_function(batch)
            self.calculate_losses_step(y, y_pred)
        else:
            self.calculate_losses_step(r[0], r[1])
            self._m().set_step_loss(r[2])
        self.log_losses("train", on_step=True)
        return self.loss


class GraphedTrainingStep:
    """One training step of a wrapper -- `optimizer.zero_grad(); loss = wrapper.training_step(batch, i); loss.backward(); optimizer.step()` -- captured ONCE in a
    HIP graph and replayed per batch.

    Why: at the reference's own batch size (32, train_regression-grf_msgn.py:93) a step is a handful of short launches and the Python between them (autograd,
    metric bookkeeping, the optimizer) costs more than the GPU work: 0.32 ms eager against 0.13 ms replayed on one MI355X.  From ~4 000 windows on the step is
    GPU-bound and the replay buys nothing.

    The graph reads its inputs from STATIC device tensors (copies of `example_batch`'s tensors, made here); `__call__(batch)` copies the new batch's tensors
    into them (same shapes and dtypes) and replays.  Everything the step touches lives on the device: the loss / metric sums (metrics.py), the flat gradient
    buffer, and the optimizer's step count -- which is why the optimizer must be `FlatAdam` / `FlatAdamW` / `FlatSGD(graph_safe=True)` (set
    `wrapper.graph_safe_optimizer = True` before `configure_optimizers()`) or a `torch.optim` optimizer created with `capturable=True`.  The model's parameters, the optimizer state and the metric
    state are restored after the warm-up steps the capture needs, so constructing this object does not train.

    Returns the step's loss as a device tensor (a static buffer: read it before the next call).

    Resuming: `optimizer.load_state_dict()` may be called after the graph was built -- FlatAdam(graph_safe=True) copies the loaded moments and step count into
    the flat buffers the captured launches address, so the next replay continues from the loaded state (restore the parameters in place as well).  lr, betas
    and eps are plain launch arguments of the captured Adam: a replay RAISES when the param group's differ from the captured values (a scheduler, a loaded
    group with another lr); build a new GraphedTrainingStep for them.  With `device_lr=True` (`wrapper.device_lr_optimizer = True`) the learning rate is
    not among them: the captured launch reads a device scalar that `__call__` refreshes from the param group before the replay, so a scheduler just works.

    `max_grad_norm`: `optim.clip_grad_norm_(wrapper.model, max_grad_norm)` is captured between `backward()` and `optimizer.step()`; `self.grad_norm` is the
    device fp64 norm (before clipping) of the last replay, a static tensor.

    `index_source` (a `windows.DatasetView`): the batch is a set of DATASET INDICES of that view.  `example_batch` is then `view.batch(indices, edge_index_dict)`
    (or anything with `indices` and `edge_index_dict`); the static input is one device int64 tensor of indices, and the captured region runs the index
    mapping (`mshgnn_dataset_starts`, which bounds every index) + the step straight from the resident series + the optimizer.  `load(indices)` /
    `__call__(indices)` copy the next batch's indices (host or device, same count) into it; `index_source.check()` tells afterwards whether any was out
    of range."""

    def __init__(self, wrapper, optimizer, example_batch, warmup: int = 3, index_source=None, max_grad_norm=None):
        import copy
        from .optim import _FlatMixin
        if _at_f64(wrapper):
            raise ValueError("GraphedTrainingStep: the model is at precision 'f64' -- its operator route builds the CSR views of the graph with host "
                             "synchronisations, which a HIP graph capture cannot contain; capture a step at 'x3', 'f32' or 'bf16'")
        flat_opt = isinstance(optimizer, _FlatMixin)      # FlatAdam, FlatAdamW, FlatSGD
        if flat_opt and not optimizer._graph_safe:
            raise ValueError(f"GraphedTrainingStep needs {type(optimizer).__name__}(graph_safe=True): set wrapper.graph_safe_optimizer = True before "
                             "configure_optimizers()")
        if not flat_opt and not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("GraphedTrainingStep needs an optimizer whose step count lives on the device (capturable=True)")
        self.wrapper, self.optimizer = wrapper, optimizer
        self.max_grad_norm, self.grad_norm = (None if max_grad_norm is None else float(max_grad_norm)), None
        self.index_source = index_source
        if index_source is not None:
            from .windows import WindowBatch
            self.indices = torch.as_tensor(example_batch.indices).to(index_source.dataset.device, torch.int64).flatten().clone()
            self._starts = index_source.starts(self.indices)      # (the static start rows the captured mapping kernel rewrites)
            self.batch = WindowBatch(index_source.dataset, self._starts, example_batch.edge_index_dict)
        else:
            self.batch = self._static_copy(example_batch)
        dev = next(wrapper.parameters()).device
        snap_p = [p.detach().clone() for p in wrapper.parameters()]
        if flat_opt:      # a flat optimizer's state lives in flat device buffers the captured launches will address: snapshot / restore them IN PLACE
            snap_o = optimizer._snapshot()
        else:
            snap_o = copy.deepcopy(optimizer.state_dict())
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self._eager_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._eager_step()
        with torch.no_grad():      # un-train: parameters and optimizer state as they were (the metric sums of the warm-up steps are cleared with the epoch's)
            for p, q in zip(wrapper.parameters(), snap_p):
                p.copy_(q)
            if flat_opt:
                if optimizer._owner is None or optimizer._t_dev is None:
                    raise RuntimeError("GraphedTrainingStep: the optimizer did not take the flat route during capture (parameters or gradients are not the flat views)")
                optimizer._restore(snap_o)
            else:
                optimizer.load_state_dict(snap_o)
        if hasattr(wrapper, "reset_all_metrics"):
            wrapper.reset_all_metrics()
        self._captured = self._optimizer_arguments()

    def _optimizer_arguments(self):
        """What the captured flat optimizer launch holds as plain arguments: lr (None with device_lr: the launch reads the device scalar) and the other
        hyperparameters of the one param group ((betas, eps, ...) of FlatAdam), then the addresses of the flat state."""
        from .optim import _FlatMixin
        o = self.optimizer
        return o._captured_arguments() if isinstance(o, _FlatMixin) else None

    @staticmethod
    def _static_copy(batch):
        import types
        out = types.SimpleNamespace()
        for k, v in vars(batch).items():
            if torch.is_tensor(v):
                setattr(out, k, v.detach().clone())
            elif isinstance(v, dict) and k == "x_dict":
                setattr(out, k, {kk: vv.detach().clone() for kk, vv in v.items()})
            else:
                setattr(out, k, v)      # edge_index_dict, batch_size, ...: the same for every batch of this size
        return out

    def _eager_step(self):
        if self.index_source is not None:
            self.index_source.starts(self.indices, out=self._starts)
            self.batch._x = self.batch._y = self.batch._q = None      # (nothing of the previous step's batch is current)
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.wrapper.training_step(self.batch, 0)
        loss.backward()
        if self.max_grad_norm is not None:
            from .optim import clip_grad_norm_
            self.grad_norm = clip_grad_norm_(self.wrapper.model, self.max_grad_norm)      # (the flat route returns one static device tensor)
        self.optimizer.step()
        return loss.detach()

    def load(self, batch):
        """Copy a batch's tensors into the static ones (host or device sources; same shapes).  With an `index_source`: `batch` is the next batch's dataset
        indices (or a batch that carries them as `indices`)."""
        if self.index_source is not None:
            ix = torch.as_tensor(batch if torch.is_tensor(batch) else getattr(batch, "indices", batch))      # (torch.Tensor has an `indices` of its own)
            if ix.numel() != self.indices.numel():
                raise ValueError(f"{ix.numel()} indices for a step captured on {self.indices.numel()}")
            self.indices.copy_(ix.reshape(self.indices.shape), non_blocking=True)
            return
        for k, v in vars(batch).items():
            dst = getattr(self.batch, k, None)
            if torch.is_tensor(v) and torch.is_tensor(dst):
                dst.copy_(v, non_blocking=True)
            elif isinstance(v, dict) and k == "x_dict":
                for kk, vv in v.items():
                    dst[kk].copy_(vv, non_blocking=True)

    def __call__(self, batch=None):
        if self._captured is not None and self._optimizer_arguments() != self._captured:
            raise RuntimeError("GraphedTrainingStep: lr, betas or eps of the optimizer's param group (or its flat state buffers) differ from what the graph "
                               f"captured: {self._optimizer_arguments()[:4]} now, {self._captured[:4]} captured; build a new GraphedTrainingStep")
        if batch is not None:
            self.load(batch)
        if self._captured is not None:
            self.optimizer._refresh_lr()      # device_lr: the scalar the captured launch reads follows param_groups[0]["lr"]
        self.graph.replay()
        self.optimizer._opt_called = True      # (the replay ran optimizer.step(): torch's lr schedulers look at this flag to warn about the call order)
        return self.loss


def tiled_edges(store, edge_index_dict):
    """batch size -> edge_index_dict for the sweeps over a store (`evaluate_sequence`, `evaluate_table`, `symmetrise.evaluate_sequence_symmetrised`): the edges of ONE
    window tiled per batch size (made once per size), or the caller's own callable batch size -> edge_index_dict."""
    r = store.recipe
    edges = {}

    def edges_for(B):
        if B not in edges:
            if callable(edge_index_dict):
                edges[B] = edge_index_dict(B)
            else:
                edges[B] = {}
                for et, ei in edge_index_dict.items():
                    ei = torch.as_tensor(ei).to(store.device)
                    off = torch.stack([torch.arange(B, device=store.device) * r.num_nodes[et[0]], torch.arange(B, device=store.device) * r.num_nodes[et[2]]])
                    edges[B][et] = (ei[:, None, :] + off[:, :, None]).reshape(2, -1)
        return edges[B]
    return edges_for


def _evaluation_sweep(wrapper, store, edge_index_dict, batch_size: int, stride: int, per_batch=None, test_only_on_z: bool = False):
    """The loop `evaluate_sequence` and `evaluate_table` share: (predictions in index order, the view swept or None).  per_batch(lo, batch, y, y_pred) runs
    after the wrapper's own metrics of every batch; lo: the batch's position in the swept indices 0, stride, 2 stride, ..."""
    if batch_size < 1 or stride < 1:
        raise ValueError("batch_size and stride must be >= 1")
    from .windows import DatasetView, ResidentDataset
    view = store.view() if isinstance(store, ResidentDataset) else store if isinstance(store, DatasetView) else None
    if view is not None:
        store = view.dataset
    starts = torch.arange(0, len(view if view is not None else store), stride, dtype=torch.int64, device=store.device)      # (a view: its indices)
    edges_for = tiled_edges(store, edge_index_dict)

    preds = []
    with torch.no_grad():
        wrapper.on_test_epoch_start()
        for i, lo in enumerate(range(0, int(starts.numel()), batch_size)):
            st = starts[lo:lo + batch_size]
            batch = (view if view is not None else store).batch(st, edges_for(int(st.numel())))
            y, y_pred = wrapper.step_helper_function(batch)
            if getattr(wrapper, "body_to_world_frame", False):
                wrapper.calculate_losses_step_worldframe(y, y_pred, batch.r_o.view(batch.batch_size, 4), test_only_on_z)
            else:
                wrapper.calculate_losses_step(y, y_pred)
            if per_batch is not None:
                per_batch(lo, batch, y, y_pred)
            preds.append(y_pred.clone())
        wrapper.on_test_epoch_end()
    if view is not None:
        view.check()
    return torch.cat(preds, 0), view


def evaluate_sequence(wrapper, store, edge_index_dict, batch_size: int, stride: int = 1) -> torch.Tensor:
    """A test epoch over every window of one sequence, in order (the loop of the reference's `evaluate_model` without its dataset plumbing): windows
    0, stride, 2 stride, ... of `store` in batches of `batch_size` (the last one ragged) through the wrapper's `test_step` under torch.no_grad() --
    with `fused_evaluation_step` straight from the resident series.  `edge_index_dict`: the edges of ONE window (tiled per batch here) or a
    callable batch size -> edge_index_dict.  Returns the predictions [n_windows, ...] in window order; the epoch's metrics are left in the
    wrapper's state (`on_test_epoch_end` has run: `wrapper.logged`, the metric attributes).

    `store` may be a `windows.DatasetView` (or a `ResidentDataset`: all of it): the view's indices 0, stride, 2 stride, ... are swept through `view.batch`,
    the predictions come back in dataset-index order."""
    return _evaluation_sweep(wrapper, store, edge_index_dict, batch_size, stride)[0]


class EvaluationTable:
    """What `evaluate_table` returns: `predictions` (exactly `evaluate_sequence`'s), `table` -- a dict of fp64 tensors [K][n_sequences], one row per
    operator and one column per sequence (`metrics.table_from_state`: regression MSE / RMSE / L1 / n, classification CE / accuracy / f1_leg_0..3 /
    f1_avg_legs / n) --, `operators` ("None", then the orbit's), `names` (the sequences') and, for classification, `totals`: the same values per
    operator over ALL sequences, [K].  With `grf_body_to_world_frame` wrappers `table_world` holds the world-frame values.

    The centroidal-momentum form (`com=True`): `table` holds `metrics.com_table_from_state`'s values (MSE, MSE_lin, MSE_ang, cos_sim_lin, cos_sim_ang,
    avg_cos_sim, n) per (operator, sequence), `totals` the same per operator over all sequences, and the CSV is the reference's
    (research/evaluator_regression-com.py:50-76): one row per operator with Test Loss (= MSE), Test Cos Sim Lin and Test Cos Sim Ang."""

    def __init__(self, predictions, table, operators, names, regression: bool = True, totals=None, table_world=None, com: bool = False):
        self.predictions, self.table, self.operators, self.names = predictions, table, list(operators), list(names)
        self.regression, self.totals, self.table_world, self.com = bool(regression), totals, table_world, bool(com)

    def header(self):
        if self.com:             # evaluator_regression-com.py:50
            return ["Symmetry Operator", "Test Loss", "Test Cos Sim Lin", "Test Cos Sim Ang"]
        if self.regression:      # evaluator_regression-grf_c2.py:170-179
            return ["Swap"] + [f"{name}-{m}" for name in self.names for m in ("MSE", "RMSE", "L1")]
        return ["Symmetry Operator", "Model Accuracy", "Rear-Left", "Front-Left", "Rear-Right", "Front-Right", "F1 Avg"]      # evaluator_classification_k4.py:52

    def rows(self):
        """One list per operator: its name, then the header's values as Python floats (one device -> host copy per column)."""
        if self.com:
            cols = [self.totals[m].detach().cpu().tolist() for m in ("MSE", "cos_sim_lin", "cos_sim_ang")]
            return [[op] + [c[k] for c in cols] for k, op in enumerate(self.operators)]
        if self.regression:
            cols = {m: self.table[m].detach().cpu().tolist() for m in ("MSE", "RMSE", "L1")}
            return [[op] + [cols[m][k][s] for s in range(len(self.names)) for m in ("MSE", "RMSE", "L1")] for k, op in enumerate(self.operators)]
        if self.totals is None:
            raise ValueError("a classification table is written from `totals` (per operator over all sequences)")
        cols = [self.totals[m].detach().cpu().tolist() for m in ("accuracy", "f1_leg_0", "f1_leg_1", "f1_leg_2", "f1_leg_3", "f1_avg_legs")]
        return [[op] + [c[k] for c in cols] for k, op in enumerate(self.operators)]

    def to_csv(self, path) -> None:
        """One row per operator, the evaluators' columns (regression: per sequence `<name>-MSE`, `<name>-RMSE`, `<name>-L1`; classification: accuracy, the
        four per-leg F1 scores and their average over all sequences; centroidal momentum: loss and the two cosine similarities over all sequences).  path: a
        file name or an open text stream."""
        import csv
        if hasattr(path, "write"):
            w = csv.writer(path, lineterminator="\n")
            w.writerow(self.header()); w.writerows(self.rows())
            return
        with open(path, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(self.header()); w.writerows(self.rows())


def evaluate_table(wrapper, view_or_dataset, edge_index_dict, batch_size: int, stride: int = 1, test_only_on_z: bool = False) -> EvaluationTable:
    """The sweep of `evaluate_sequence` over a `windows.DatasetView` (or a `ResidentDataset`: all of it) that ALSO keeps the metrics per (operator, sequence):
    every window carries the segment id element * n_sequences + sequence (`DatasetView.segments`) and one `metrics.SegmentedMetrics.update` per batch adds
    its sums to that row -- the evaluators' whole table (one CSV row per symmetry operator, research/evaluator_regression-grf_c2.py:170-221,
    evaluator_classification_k4.py:57-89) out of one pass over an `orbit` view, with no host read until the sweep is over.  The wrapper's own epoch metrics
    are left in its state as `evaluate_sequence` leaves them.  With `grf_body_to_world_frame` a second table is kept on the rotated pairs (`test_only_on_z`
    as in `calculate_losses_step_worldframe`).

    The centroidal-momentum (COM) wrappers, over a view of Solo recipes (an `orbit` of `symmetry=True` recipes, or a plain dataset: one row): the same sweep
    with `metrics.SegmentedComMetrics` per (operator, sequence) -- the table research/evaluator_regression-com.py:50-76 writes, one row per operator."""
    from .metrics import SegmentedComMetrics, SegmentedMetrics, com_table_from_state, table_from_state
    from .windows import DatasetView, ResidentDataset
    com = isinstance(wrapper, COM_Base_Lightning)
    if isinstance(view_or_dataset, ResidentDataset):
        view_or_dataset = view_or_dataset.view()
    if not isinstance(view_or_dataset, DatasetView):
        if com:
            raise ValueError("evaluate_table takes the centroidal-momentum (COM) wrappers over a windows.DatasetView or a windows.ResidentDataset only")
        raise TypeError("evaluate_table takes a windows.DatasetView or a windows.ResidentDataset")
    view = view_or_dataset
    K, S = view.segment_shape
    regression = bool(wrapper.regression)
    world = bool(getattr(wrapper, "body_to_world_frame", False))
    if com:
        seg_m = SegmentedComMetrics(K * S, wrapper.model.num_bases, *wrapper.__dict__["_stats"], device=view.dataset.device)
    else:
        seg_m = SegmentedMetrics(K * S, regression, device=view.dataset.device)
    seg_w = SegmentedMetrics(K * S, True, device=view.dataset.device) if world else None
    seg_m.reserve(batch_size)
    if world:
        seg_w.reserve(batch_size)

    # the ids of the whole sweep in one go (a handful of torch integer ops on the device), a slice of them per batch
    seg_all = view.segments(torch.arange(0, len(view), stride, dtype=torch.int64, device=view.dataset.device))

    def per_batch(lo, batch, y, y_pred):
        seg = seg_all[lo:lo + batch.batch_size]
        seg_m.update(y, y_pred, seg)
        if world:
            q = batch.r_o.view(batch.batch_size, 4)
            y_w, p_w = wrapper.body_frame_to_world_frame(q, y.detach()), wrapper.body_frame_to_world_frame(q, y_pred.detach())
            if test_only_on_z:
                y_w, p_w = y_w[:, [2, 5, 8, 11]], p_w[:, [2, 5, 8, 11]]
            seg_w.update(y_w, p_w, seg)

    preds, _ = _evaluation_sweep(wrapper, view, edge_index_dict, batch_size, stride, per_batch, test_only_on_z)
    seg_m.check()
    shape = lambda t: {k: v.view(K, S) for k, v in t.items()}
    totals = None
    if com:
        totals = com_table_from_state(seg_m.state[:K * S].view(K, S, 8).sum(1))
    elif not regression:
        n = K * S
        totals = table_from_state(seg_m.state[:n].view(K, S, 2).sum(1), seg_m.counts[:n].view(K, S, 18).sum(1))
    ops = ["None" if op is None else str(op) for op in getattr(view.dataset, "operators", [None])]
    res = EvaluationTable(preds, shape(seg_m.table()), ops, view.names, regression, totals, shape(seg_w.table()) if world else None, com)
    res.metrics, res.metrics_world = seg_m, seg_w
    return res
