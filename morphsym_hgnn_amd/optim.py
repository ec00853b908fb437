"""torch's optimizers for a model whose parameters live in the engine's flat buffer: the whole update is ONE launch.

`configure_optimizers` of the reference's wrappers returns `optim.Adam(self.parameters(), lr)` or `optim.SGD(self.parameters(), lr)` (gnnLightning.py:258-265).
With this package's models the parameters are views of one flat fp32 buffer and their `.grad`s are views of one flat gradient buffer
(`models._MSHGNNBase._flat_params`, `_deliver_gradients`), so the ~50 per-tensor (or multi-tensor) kernels of torch's optimizers collapse into one sweep
over the two flat buffers:

  FlatAdam   torch.optim.Adam.  Defaults: `mshgnn_adam_step` / `mshgnn_adam_step_counted`; with weight_decay != 0 (coupled: the decay enters the moments) or
             device_lr: `mshgnn_adamw_step(decoupled=0)`.
  FlatAdamW  torch.optim.AdamW (decoupled decay: p *= 1 - lr wd): `mshgnn_adamw_step(decoupled=1)`.
  FlatSGD    torch.optim.SGD with momentum / dampening / nesterov / weight decay: `mshgnn_sgd_step`, one flat momentum buffer.

The bias corrections 1 - beta^t are formed in double, as torch forms them, and rounded to fp32 once; the moments and the update itself are fp32 arithmetic,
every element within a few units of 2^-24 of the fp64 value of one step (the bounds of tests/train_ops_reference.py and tests/optim_reference.py, held per
element in tests/test_train_ops_exact_gpu.py and tests/test_optim_exact_gpu.py; whole runs are compared with torch's optimizers in tests/test_engine_gpu.py,
tests/test_wrappers.py and tests/test_flat_optim_gpu.py).

Each of them IS its torch optimizer (same constructor defaults, `param_groups`, `state_dict()` / `load_state_dict()` with torch's own per-parameter
layout, `zero_grad`); whenever the flat layout is not in place at `step()` -- parameters moved or re-created, gradients that are not the flat views (DDP
buckets, a parameter without gradient), amsgrad / maximize / foreach / fused / differentiable switched on, a tensor lr, more than one parameter group -- it
carries its state over and runs torch's own step.

graph_safe: the step count lives on the device, so `step()` can be captured in a HIP graph and replayed (wrappers.GraphedTrainingStep) -- the flat route's
counterpart of capturable=True.  The flat state buffers are allocated once and then only written in place: `load_state_dict` and a re-adoption copy into them.
device_lr: the learning rate lives in a device fp32 scalar that `step()` refreshes (a fill on the step's stream) whenever `param_groups[0]["lr"]` has
changed, and the launch reads it there: a captured step follows a scheduler.

`clip_grad_norm_(model, max_norm)`: `torch.nn.utils.clip_grad_norm_` on the flat gradient -- `mshgnn_grad_norm` + `mshgnn_grad_clip`, two launches, capturable.
"""
from __future__ import annotations

import weakref

import torch

from . import engine as eng


class _FlatMixin:
    """What the flat optimizers share: the route decision, adopt / publish / sync of the flat state, the device-resident step count and learning rate, and
    the rule that graph_safe fills existing buffers in place and never re-allocates them.  A subclass names torch's per-parameter state keys that are backed
    by one flat buffer each (`_state_keys`), reads / writes one parameter's entry (`_read_entry`, `_entry`) and launches (`_launch`)."""

    def _flat_init(self, model, graph_safe, device_lr):
        self._model = model
        self._graph_safe = bool(graph_safe)
        self._device_lr = bool(device_lr)
        self._t_dev = None                # graph_safe: device int64 step count (the truth; self._t is refreshed from it when the state is published)
        self._bufs = []                   # the flat state buffers, one per state key (the per-parameter state entries are views of them)
        self._t = 0                       # steps taken on the flat route since the state was last synchronised with self.state
        self._owner = None                # the flat parameter buffer the flat state belongs to
        self._lr_dev = None               # device_lr: device fp32[1], and the host value it was last filled with
        self._lr_host = None

    # ---- which route --------------------------------------------------------------------------------------------------
    _TORCH_ONLY = ()                      # param-group switches that send the step to torch's own code

    def _flat_route(self):
        m = self._model
        if len(self.param_groups) != 1:
            return None
        g = self.param_groups[0]
        if any(g.get(k) for k in self._TORCH_ONLY) or isinstance(g["lr"], torch.Tensor):
            return None
        flat, gflat, gviews, params = getattr(m, "_flat", None), getattr(m, "_gflat", None), getattr(m, "_gviews", None), getattr(m, "_param_list", None)
        if not getattr(m, "_flat_ok", False) or flat is None or gflat is None or gviews is None or params is None or not flat.is_cuda:
            return None
        if len(params) != len(g["params"]) or any(a is not b for a, b in zip(params, g["params"])):
            return None
        if any(p.grad is not v for p, v in zip(params, gviews)):
            return None
        return flat, gflat, params, g

    # ---- state: flat buffers <-> torch's per-parameter entries -------------------------------------------------------------
    def _offsets(self):
        return list(self._model._spec.param_offsets().values())

    def _adopt(self, flat, params):
        """Start (or re-start, after the model re-created its flat buffer or a state was loaded) the flat state from whatever torch-layout state exists.
        graph_safe: once the flat buffers and `_t_dev` exist (and fit the flat buffer) they are FILLED IN PLACE, never re-allocated -- a captured step
        (wrappers.GraphedTrainingStep) addresses them."""
        keys = self._state_keys(self.param_groups[0])
        bufs = [torch.zeros_like(flat) for _ in keys]      # (filled first: the entries read below may be views of the buffers that are kept)
        steps = set()
        for (o, n), p in zip(self._offsets(), params):
            t = self._read_entry(self.state.get(p), [b[o:o + n] for b in bufs])
            if t is not None:
                steps.add(t)
        if len(steps) > 1:
            raise RuntimeError(self._MIXED_STATE)
        keep = self._graph_safe and self._t_dev is not None and len(self._bufs) == len(bufs) \
            and all(b.shape == flat.shape and b.device == flat.device for b in self._bufs) and self._t_dev.device == flat.device
        if keep:
            for dst, src in zip(self._bufs, bufs):
                dst.copy_(src)
        else:
            self._bufs = bufs
        self._t, self._owner = (steps.pop() if steps else 0), flat
        if self._graph_safe:
            if keep:
                self._t_dev.fill_(self._t)
            else:
                self._t_dev = torch.tensor([self._t], dtype=torch.int64, device=flat.device)
        self._publish(params)

    def _publish(self, params):
        """torch's per-parameter state entries as VIEWS of the flat buffers (so state_dict() and a later torch-route step see them)."""
        for (o, n), p in zip(self._offsets(), params):
            st = self._entry([b[o:o + n].view(p.shape) for b in self._bufs])
            if st is None:
                self.state.pop(p, None)
            else:
                self.state[p] = st

    def _sync_steps(self):
        if self._graph_safe and self._t_dev is not None and self._owner is not None:
            self._t = int(self._t_dev.item())      # (a host sync: state_dict / route changes only, never inside a captured step)
        if self._owner is not None:
            self._republish()

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """graph_safe, with the flat state in place: the loaded state and step count are copied INTO the existing flat buffers at once (a captured step keeps
        addressing them, so a checkpoint loaded after the graph was built takes effect at the next replay).  The hyperparameters are launch arguments of a
        captured step (lr too, unless device_lr): GraphedTrainingStep refuses to replay when the loaded group's differ from the captured ones."""
        owner = self._owner
        super().load_state_dict(state_dict)
        self._owner = None                # re-adopt from the loaded per-parameter state at the next step
        params = getattr(self._model, "_param_list", None)
        if self._graph_safe and owner is not None and self._t_dev is not None and params is not None and len(self.param_groups) == 1 \
                and len(params) == len(self.param_groups[0]["params"]) and all(a is b for a, b in zip(params, self.param_groups[0]["params"])):
            with torch.no_grad():
                self._adopt(owner, params)

    # ---- what wrappers.GraphedTrainingStep needs: the flat state saved and put back IN PLACE, and what a captured launch holds as plain arguments -------
    def _snapshot(self):
        self._sync_steps()
        return None if self._owner is None else ([b.clone() for b in self._bufs], int(self._t))

    def _restore(self, snap):
        bufs, t = snap if snap is not None else ([torch.zeros_like(b) for b in self._bufs], 0)
        if len(bufs) != len(self._bufs):
            raise RuntimeError("the optimizer's flat state changed its layout during the capture")
        for dst, src in zip(self._bufs, bufs):
            dst.copy_(src)
        self._t = t
        self._t_dev.fill_(t)
        self._sync_steps()

    def _captured_arguments(self):
        g = self.param_groups[0]
        hp = self._hyperparameters(g)
        return (None if self._device_lr else float(g["lr"]),) + tuple(hp) + tuple(b.data_ptr() for b in self._bufs) \
            + (self._t_dev.data_ptr(), self._lr_dev.data_ptr() if self._lr_dev is not None else None)

    # ---- the learning rate on the device -------------------------------------------------------------------------------------
    def _refresh_lr(self, device=None):
        """device_lr: the device scalar holds fl32(param_groups[0]["lr"]) -- allocated once, re-filled (on the current stream) when the host value changed."""
        if not self._device_lr:
            return None
        lr = float(self.param_groups[0]["lr"])
        if self._lr_dev is None:
            self._lr_dev = torch.full((1,), lr, dtype=torch.float32, device=device if device is not None else self._owner.device)
        elif lr != self._lr_host:
            self._lr_dev.fill_(lr)
        self._lr_host = lr
        return self._lr_dev

    # ---- step ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        route = self._flat_route()
        if route is None:
            self._sync_steps()
            self._owner = None               # (the per-parameter entries stay views of the old flat state; a return to the flat route re-adopts them)
            super().step()
            return loss
        flat, gflat, params, g = route
        if self._owner is not flat or len(self._bufs) != len(self._state_keys(g)):
            if self._owner is flat:
                self._sync_steps()
            self._adopt(flat, params)
        lr_dev = self._refresh_lr(flat.device)
        if not self._graph_safe:
            self._t += 1
        with torch.cuda.device(flat.device):
            self._launch(eng.load_library(), flat, gflat, g, self._t, self._t_dev.data_ptr() if self._graph_safe else None,
                         lr_dev.data_ptr() if lr_dev is not None else None, torch.cuda.current_stream(flat.device).cuda_stream)
        if self._t == 1 and not self._graph_safe:
            self._first_step_taken()
        return loss

    def _first_step_taken(self):
        pass


class _FlatAdamMixin(_FlatMixin):
    _MIXED_STATE = "FlatAdam: the parameters' step counts differ; use torch.optim.Adam for this state"
    _TORCH_ONLY = ("amsgrad", "maximize", "capturable", "differentiable")
    _DECOUPLED = False

    # FlatAdam's names for the two flat moments
    _m = property(lambda self: self._bufs[0] if self._bufs else None)
    _v = property(lambda self: self._bufs[1] if self._bufs else None)

    def _state_keys(self, g):
        return ("exp_avg", "exp_avg_sq")

    def _read_entry(self, st, slices):
        if not st:
            return None
        slices[0].copy_(st["exp_avg"].reshape(-1))
        slices[1].copy_(st["exp_avg_sq"].reshape(-1))
        return int(st["step"])

    def _entry(self, views):
        return {"step": torch.tensor(float(self._t)), "exp_avg": views[0], "exp_avg_sq": views[1]}

    def _republish(self):
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(float(self._t))

    def _hyperparameters(self, g):
        return float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g.get("weight_decay", 0)), self._decoupled(g)

    def _decoupled(self, g):
        return bool(self._DECOUPLED or g.get("decoupled_weight_decay", False))

    def _launch(self, lib, flat, gflat, g, t, t_dev, lr_dev, stream):
        b1, b2, eps, wd, decoupled = self._hyperparameters(g)
        m, v = self._bufs
        if wd == 0 and lr_dev is None:      # torch.optim.Adam's defaults: the two entry points this class has always called
            if t_dev is not None:
                eng._check(lib, lib.mshgnn_adam_step_counted(flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), flat.numel(), t_dev, float(g["lr"]),
                                                             b1, b2, eps, 1.0, stream), "mshgnn_adam_step_counted")
            else:
                eng._check(lib, lib.mshgnn_adam_step(flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), flat.numel(), t, float(g["lr"]),
                                                     b1, b2, eps, 1.0, stream), "mshgnn_adam_step")
            return
        eng._check(lib, lib.mshgnn_adamw_step(flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), flat.numel(), max(int(t), 1), t_dev, float(g["lr"]),
                                              lr_dev, b1, b2, eps, wd, int(decoupled), 1.0, stream), "mshgnn_adamw_step")


class FlatAdam(_FlatAdamMixin, torch.optim.Adam):
    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, graph_safe: bool = False, device_lr: bool = False, **kw):
        """graph_safe: the step count lives on the device (`mshgnn_adam_step_counted`), so `step()` can be captured in a HIP graph and replayed
        (wrappers.GraphedTrainingStep) -- the flat route's counterpart of torch.optim.Adam(capturable=True).  Its flat state buffers (`_m`, `_v`, `_t_dev`) are
        allocated once and then only written in place: `load_state_dict` and a re-adoption copy into them.  device_lr: see the module docstring."""
        super().__init__(model.parameters(), lr=lr, betas=betas, eps=eps, **kw)
        self._flat_init(model, graph_safe, device_lr)


class FlatAdamW(_FlatAdamMixin, torch.optim.AdamW):
    _MIXED_STATE = "FlatAdamW: the parameters' step counts differ; use torch.optim.AdamW for this state"
    _DECOUPLED = True

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, graph_safe: bool = False,
                 device_lr: bool = False, **kw):
        super().__init__(model.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self._flat_init(model, graph_safe, device_lr)


class FlatSGD(_FlatMixin, torch.optim.SGD):
    """torch.optim.SGD on the flat buffers.  With momentum there is ONE flat momentum buffer; `state[p]["momentum_buffer"]` are views of it once a step has
    been taken and None before, as torch has it.  `_t` counts what the update needs to know: 0 before the first step (the buffer is then only written), and
    not 0 afterwards (a state adopted from torch's layout carries no count: 1)."""
    _MIXED_STATE = "FlatSGD: some parameters have a momentum buffer and some have none; use torch.optim.SGD for this state"
    _TORCH_ONLY = ("maximize", "foreach", "fused", "differentiable")

    def __init__(self, model, lr: float = 1e-3, momentum: float = 0, dampening: float = 0, weight_decay: float = 0, nesterov: bool = False,
                 graph_safe: bool = False, device_lr: bool = False, **kw):
        super().__init__(model.parameters(), lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._flat_init(model, graph_safe, device_lr)

    def _state_keys(self, g):
        return ("momentum_buffer",) if g["momentum"] != 0 else ()

    def _read_entry(self, st, slices):
        if not slices:
            return None
        buf = st.get("momentum_buffer") if st else None
        if buf is None:
            return 0
        slices[0].copy_(buf.reshape(-1))
        return 1

    def _entry(self, views):
        if not views:
            return None
        return {"momentum_buffer": views[0] if self._t > 0 else None}

    def _republish(self):
        params = getattr(self._model, "_param_list", None)
        if params is not None and self._bufs:
            self._publish(params)

    _first_step_taken = _republish      # (graph_safe: the entries turn from None into the views at the next state_dict() / _sync_steps())

    def _hyperparameters(self, g):
        return float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"]), bool(g["nesterov"])

    def _launch(self, lib, flat, gflat, g, t, t_dev, lr_dev, stream):
        mom, damp, wd, nesterov = self._hyperparameters(g)
        eng._check(lib, lib.mshgnn_sgd_step(flat.data_ptr(), gflat.data_ptr(), self._bufs[0].data_ptr() if self._bufs else None, flat.numel(), max(int(t), 1),
                                            t_dev, float(g["lr"]), lr_dev, mom, damp, wd, int(nesterov), 1.0, stream), "mshgnn_sgd_step")


_CLIP_STATE = weakref.WeakKeyDictionary()      # model -> (the flat gradient buffer it belongs to, the norm [1] fp64, the ticket scratch)


def clip_grad_norm_(model, max_norm: float) -> torch.Tensor:
    """`torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)` (norm_type 2): the gradients are scaled in place by min(1, max_norm / (norm + 1e-6))
    and the total norm BEFORE clipping is returned as a device fp64 tensor.  With the gradients being the flat views it is `mshgnn_grad_norm` +
    `mshgnn_grad_clip` on `model._gflat` -- two launches, no host synchronisation, capturable in a HIP graph; the returned tensor is then a static buffer kept
    per model (read it before the next call).  Otherwise torch's own function runs."""
    gflat, gviews, params = getattr(model, "_gflat", None), getattr(model, "_gviews", None), getattr(model, "_param_list", None)
    if gflat is None or gviews is None or params is None or not gflat.is_cuda or not getattr(model, "_flat_ok", False) \
            or len(params) != len(list(model.parameters())) or any(p.grad is not v for p, v in zip(params, gviews)):
        return torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm).double()
    lib = eng.load_library()
    st = _CLIP_STATE.get(model)
    if st is None or st[0] is not gflat:
        words = (lib.mshgnn_grad_norm_scratch_bytes(gflat.numel()) + 7) // 8
        st = (gflat, torch.zeros(1, dtype=torch.float64, device=gflat.device), torch.zeros(words, dtype=torch.int64, device=gflat.device))
        _CLIP_STATE[model] = st
    _, norm, scratch = st
    stream = torch.cuda.current_stream(gflat.device).cuda_stream
    with torch.cuda.device(gflat.device):
        eng._check(lib, lib.mshgnn_grad_norm(gflat.data_ptr(), gflat.numel(), norm.data_ptr(), scratch.data_ptr(), stream), "mshgnn_grad_norm")
        eng._check(lib, lib.mshgnn_grad_clip(gflat.data_ptr(), gflat.numel(), norm.data_ptr(), float(max_norm), stream), "mshgnn_grad_clip")
    return norm
