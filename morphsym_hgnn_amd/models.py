"""Drop-in model surface of the MS-HGNN hot path: `GRF_HGNN_C2`, `GRF_HGNN_K4`, `GRF_HGNN` with the reference's
constructor signatures, attributes, parameter names and `forward(x_dict, edge_index_dict) -> Tensor` contract
(src/ms_hgnn/lightning_py/hgnn_c2.py:10-12,133; hgnn_k4.py:10-11,146; hgnn.py:10-12,57), so the Lightning wrappers
(gnnLightning.py:564-722) and the research scripts run unchanged on top of it.

All arithmetic runs in the HIP engine behind the C-ABI (engine.py / include/mshgnn.h).  The first forward
(the wrapper's lazy-init call under no_grad, gnnLightning.py:593-595) materialises the lazy encoder weights,
recovers the per-window topology from the PyG-batched `edge_index_dict`, verifies the batch really is B copies
of one graph, and compiles a plan; later calls reuse it.  Precision: `MSHGNN_DTYPE=x3` (default: the split-bf16 parity plan,
<= 1.4e-5 of the fp64 reference against the north_star's 1e-4, at 3.6x the speed of `f32`), `f32` (exact fp32 MFMA, 1e-6) or `bf16`
(throughput mode, 4.6e-3); `model.set_precision("bf16")` switches at run time.  A fourth precision, `f64`, is the reference's own (fp64 parameters, fp64 MFMA
operators under `_forward_operators`, no fused engine): `_MSHGNNBase.set_precision`.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch
import yaml
from torch import nn
from torch.autograd.function import once_differentiable

from . import nn as pnn
from .spec import ModelSpec, rel_key
from .engine import accepted_pitches
from .topology import NODE_TYPES, RobotTopology, infer_window_edges


def _fill_flat(flat, offsets, params):
    """Copy the parameters into their slices of a flat fp32 buffer (state_dict order, the C-ABI's layout); returns the slices as views of the parameters' shapes."""
    views = [flat[o:o + n].view(p.shape) for (o, n), p in zip(offsets, params)]
    torch._foreach_copy_(views, [p.detach() for p in params])
    return views


class _Flatten(torch.autograd.Function):
    """named parameters -> the C-ABI's flat fp32 buffer; backward hands each parameter a view of the flat
    gradient (cast back to the parameter's dtype)."""

    @staticmethod
    def forward(ctx, size, device, offsets, *params):
        ctx.offsets = offsets
        ctx.meta = [(p.shape, p.dtype, p.device) for p in params]
        flat = torch.zeros(size, dtype=torch.float32, device=device)
        _fill_flat(flat, offsets, params)
        return flat

    @staticmethod
    def backward(ctx, gflat):
        grads = []
        for (o, n), (shape, dt, dev) in zip(ctx.offsets, ctx.meta):
            grads.append(gflat[o:o + n].view(shape).to(device=dev, dtype=dt))
        return (None, None, None, *grads)


def _check_stash(engine, B, ticket):
    if engine.stash_ticket(B) != ticket:
        raise RuntimeError("the activation stash of this forward was overwritten by a later forward of the same "
                           "batch size on the same engine; call backward before the next forward")


class _EngineFn(torch.autograd.Function):
    """The two-call route of forward(): engine.forward here, engine.backward (and mshgnn_input_grad) in backward.  Double backward is not supported on any route.
    cfg: (model, engine, B, flat, cast inputs, route, number of parameter tensors); tensors: (*parameter tensors, *caller's inputs).  The parameters travel by `route`:
      "fast": single process, parameters are device views of the flat buffer.  Their gradients do not travel through autograd at all -- 50 AccumulateGrad nodes and
              50 freshly sliced views per step cost more host time than the whole step takes on the GPU: the C-ABI writes the flat gradient into a persistent buffer
              whose per-parameter views are cached (_deliver_gradients).  The one parameter tensor is the model's `_anchor`, there only so that the output requires grad.
      "p":    the same device views under torch.distributed, as autograd inputs: DistributedDataParallel needs the per-parameter autograd hooks.  Backward hands every
              parameter a VIEW of the flat gradient (no per-parameter cast or copy kernels), in a fresh buffer per backward so that .grad views never alias; under
              ddp.flat_data_parallel no DDP wrapper hooks the parameters and the flat gradient is exchanged here (_MSHGNNBase._flat_exchange).
      "flat": host parameters; the one parameter tensor is their _Flatten output, which stands in for cfg's flat buffer.
      None:   every parameter frozen -- the backward passes no gradient buffer (activation backward only) and no .grad is touched.
    The caller's x_dict tensors are autograd inputs iff one of them requires grad (the engine's cast / re-pitched copies stay out of the graph); backward then returns
    each one its gradient -- same shape, dtype and device -- from mshgnn_input_grad (models the reference's autograd through apply_symmetry and the encoder,
    hgnn_c2.py:150-151).  Otherwise none is passed and mshgnn_input_grad is not called."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        model, engine, B, flat, xs, route, n_p = cfg
        if route == "flat":
            flat = tensors[0]
        out = engine.forward(xs, flat, B, training=True)
        ctx.cfg, ctx.flat, ctx.ticket = cfg, flat, engine.stash_ticket(B)
        ctx.shapes = [p.shape for p in tensors[:n_p]]
        ctx.xin = [(x.shape, x.dtype, x.device, x.requires_grad) for x in tensors[n_p:]]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        model, e, B, _, xs, route, n_p = ctx.cfg
        flat = ctx.flat
        _check_stash(e, B, ctx.ticket)
        g32 = gout.contiguous().to(torch.float32)
        pgrads = [None] * n_p
        if route is None:
            e.backward(xs, flat, g32, B, weights=False)
        elif route == "fast":
            _deliver_gradients(model, flat, lambda target: e.backward(xs, flat, g32, B, grad_flat=target))
        elif route == "flat":
            pgrads = [e.backward(xs, flat, g32, B)]
        else:
            n_flat = flat.numel()
            full = torch.empty(n_flat + 16, dtype=torch.float32, device=flat.device)      # a fresh buffer per backward: .grad views never alias
            gflat = e.backward(xs, flat, g32, B, grad_flat=full[:n_flat])
            div = model._flat_exchange(full, n_flat, B)
            if div is not None:
                gflat.div_(div)
            pgrads = [gflat[o:o + n].view(shape) for (o, n), shape in zip(model._spec.param_offsets().values(), ctx.shapes)]
        if not ctx.xin:
            return (None, *pgrads)
        want = [t for t, (_, _, _, rg) in zip(e.types, ctx.xin) if rg]
        direct = {t: dt for t, (shape, dt, dev, _) in zip(e.types, ctx.xin) if dt in (torch.float32, torch.float64)}
        pitches = {t: shape[1] for t, (shape, _, _, _) in zip(e.types, ctx.xin)}
        by_dtype = {}
        for t in want:
            by_dtype.setdefault(direct.get(t, torch.float32), []).append(t)
        g = {}
        for dt, ts in by_dtype.items():      # one launch per output dtype (one in practice: x_dict tensors share theirs)
            g.update(e.input_grad(B, flat, ts, dt, pitches))
        xgrads = [g[t].to(device=dev, dtype=dt) if t in g else None for t, (_, dt, dev, _) in zip(e.types, ctx.xin)]
        return (None, *pgrads, *xgrads)


def _several_processes():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _window_recipe_ok(spec, r, desc, dtype, training):
    """The device-free part of `_MSHGNNBase._window_route`: can a store of this recipe, descriptor and dtype feed the series entry points of a model with `spec`
    (training: mshgnn_step_*_series[_std]; evaluation: mshgnn_forward_series)?  Mirrors what the library's check_window_desc refuses, so that such a batch is
    assembled instead of raising."""
    if spec is None or dtype not in ("bf16", "x3", "f32") or not desc.fast_layout:      # (spec None: the model has not seen its lazy-initialising forward yet)
        return False
    if r.normalize and not 2 <= r.history <= 256:      # (what the standardising encoders refuse)
        return False
    if list(r.node_types) != list(spec.node_types) or any(r.num_nodes[t] != spec.num_nodes[t] or r.width(t) != spec.widths[t] for t in r.node_types):
        return False
    if training and not r.label_cols:      # the training steps compute the loss from the recipe's labels; evaluation runs without
        return False
    # Node rows of several runs need history >= 8 (the encoders take a chunk's 8 elements from at most two runs): the Solo recipes.  Evaluation and the standardised
    # training steps check it.  The plain training steps lack the check, in the library (several_runs_need_history8 = false there) and therefore here: closing that
    # changes what the wrappers must fall back on and belongs in a change of its own.
    if r.history < 8 and desc.n_runs > desc.n_rows and (r.normalize or not training):
        return False
    return True


def _deliver_gradients(m, flat, fresh, scale=None):
    """Hand a freshly computed flat gradient to the parameters' .grad (views of the persistent m._gflat): assigned when the gradients were
    cleared (zero_grad(set_to_none=True), the first step), ADDED otherwise -- what autograd's accumulation would have produced.  Decided per
    TRAINABLE parameter: a frozen parameter's .grad stays None and says nothing; a .grad that is not this buffer's view (left over from
    before a .to() re-created the flat buffers, or assigned by another route) is accumulated into in place, like autograd would.
    fresh: callable(target | None) -> the flat gradient, written into `target` when given."""
    params = m._param_list
    if m._gflat is None or m._gflat.device != flat.device:
        m._gflat = torch.zeros_like(flat)
        m._gviews = [m._gflat[o:o + n].view(p.shape) for (o, n), p in zip(m._spec.param_offsets().values(), params)]
    trainable = [(p, v) for p, v in zip(params, m._gviews) if p.requires_grad]
    if all(p.grad is None for p, _ in trainable):      # every gradient was cleared: the buffer is free to be overwritten
        fresh(m._gflat)
        if scale is not None:
            m._gflat.mul_(scale)
        for p, v in trainable:
            p.grad = v
        return
    g = fresh(None)
    if scale is not None:
        g = g * scale
    if all(p.grad is v for p, v in trainable):         # accumulation into the views of this buffer: one flat add
        m._gflat.add_(g)
        return
    for (p, v), (o, n) in zip(zip(params, m._gviews), m._spec.param_offsets().values()):
        if not p.requires_grad:
            continue
        gp = g[o:o + n].view(p.shape)
        if p.grad is None:           # cleared individually: takes the view, holding exactly this step's gradient
            v.copy_(gp)
            p.grad = v
        elif p.grad is v:
            v.add_(gp)
        else:                        # a foreign gradient tensor (stale view of an earlier buffer, a user-assigned tensor): accumulate in place
            p.grad.add_(gp.to(p.grad.dtype))


class _FusedStepFn(torch.autograd.Function):
    """_MSHGNNBase.fused_training_step: the whole step (forward, wrapper loss, backward) runs in forward() as one engine call that leaves the
    flat gradient in a pending buffer; backward() hands it to the parameters times the upstream factor (Lightning clears the gradients
    BETWEEN training_step and backward, so nothing may touch .grad before).  target: fp32 labels (regression) or int32 contact flags."""

    @staticmethod
    def forward(ctx, anchor, model, run):
        """run(grad_flat) -> (out, loss[1]): the engine call (mshgnn_step_mse / _ce or their *_series forms)."""
        if model._gpend is None or model._gpend.device != model._flat.device:
            n = model._flat.numel()      # (+ spare elements: the window count of ddp.exchange_flat_gradient_ rides behind the gradient)
            model._gpend_full = torch.empty(n + 16, dtype=torch.float32, device=model._flat.device)
            model._gpend = model._gpend_full[:n]
        out, loss = run(model._gpend)
        model._gpend_id += 1
        ctx.model, ctx.flat, ctx.ticket = model, model._flat, model._gpend_id
        ctx.windows = out.shape[0] // max(1, model._spec.num_nodes[model._spec.out_type])
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)      # (no zero tensor for the output's absent gradient)
        return loss[0], out

    @staticmethod
    def backward(ctx, gl, _gout):
        m = ctx.model
        n_in = len(ctx.needs_input_grad)
        if gl is None:
            return (None,) * n_in
        if m._gpend_id != ctx.ticket:
            raise RuntimeError("the pending gradient of this training step was overwritten by a later fused training step of the same "
                               "model; call backward before the next step")
        pend, scale = m._gpend, gl.to(device=m._gpend.device, dtype=torch.float32)
        div = m._flat_exchange(m._gpend_full, pend.numel(), ctx.windows)
        if div is not None:
            scale = scale / div
        _deliver_gradients(m, ctx.flat, lambda target: torch.mul(pend, scale, out=target) if target is not None else pend * scale)
        return (None,) * n_in


class _MSHGNNBase(nn.Module):
    kind = "c2"
    num_bases = 2

    def _init_common(self, hidden_channels, num_layers, data_metadata, regression, activation_fn):
        # The fused engines implement the reference's default, nn.ReLU().  Any other activation module
        # (the constructors accept one, hgnn_c2.py:10-12) runs the same forward operator by operator on the stand-alone HIP operators
        # of ops.py (_forward_operators): PyG-style launches instead of the fused kernels -- slower, same numerics, still no CPU path.
        self._fused_activation = isinstance(activation_fn, nn.ReLU)      # (any hidden width: the engines' widths are multiples of 128, other widths run
                                                                       #  zero-padded to the next one -- engine.PaddedEngine -- with identical results)
        self.regression = regression
        self.activation = activation_fn
        self.hidden_channels = hidden_channels
        self.num_layers = num_layers
        self._node_types = list(data_metadata[0])
        self._edge_types = [tuple(e) for e in data_metadata[1]]
        self._engines: Dict[Tuple[str, str], object] = {}
        self._spec: Optional[ModelSpec] = None
        self._flat: Optional[torch.Tensor] = None
        self._flat_ok = False            # parameters are fp32 views into self._flat (device-resident fast path)
        self._param_list = None
        self._gflat = None               # persistent flat gradient + its cached per-parameter views (_EngineFn's "fast" route)
        self._gpend = None               # the flat gradient a fused training step computed, until its backward() delivers it
        self._gpend_id = 0
        self._flat_ddp = None            # ddp.flat_data_parallel: the process group the fused training step all-reduces its flat gradient over
        self._flat_ddp_weighted = False  # ... True: each rank's gradient weighted by its window count (opt-in; the default is DDP's mean of the ranks' means)
        self._flat_ddp_live = None       # ... over the live elements only (flat_data_parallel(live_only=True)): (index, packed buffer)
        self._gpend_full = None
        self._gviews = None
        self._anchor = None
        self._checked_batches = set()
        self._precision = os.environ.get("MSHGNN_DTYPE", "x3")      # ("f64": the constructors finish with _adopt_env_precision, once the parameters exist)
        self._group = None
        self._reg_loss = ("mse", 1.0)    # set_regression_loss: what the regression routes train on (kept here for the "f64" precision and for engines compiled later)

    # ---- copy / pickle: compiled plans (ctypes handles) and device scratch never travel; they are rebuilt lazily ----
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engines"] = {}
        state["_flat"] = None
        state["_flat_ok"] = False
        state["_gflat"] = state["_gviews"] = state["_anchor"] = state["_gpend"] = state["_gpend_full"] = state["_flat_ddp"] = state["_flat_ddp_live"] = None
        state["_param_list"] = None
        state["_checked_batches"] = set()
        return state

    def zero_grad(self, set_to_none: bool = True) -> None:
        """nn.Module.zero_grad walks the whole module tree (~0.3 ms of host time for these ~80 sub-modules: as long as the GPU step);
        same semantics over the cached parameter list."""
        if self._spec is None:
            return super().zero_grad(set_to_none)
        for p in self._params_in_flat_order():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:      # (torch.optim's zero_grad: .grad tensors here are views of the flat gradient buffer, which detach_() refuses)
                    if p.grad.grad_fn is not None:
                        p.grad.detach_()
                    else:
                        p.grad.requires_grad_(False)
                    p.grad.zero_()

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .double() / .float() replace the parameter tensors: the flat-buffer views are re-established by the next forward
        self._flat_ok = False
        return super()._apply(fn, *args, **kwargs)

    def _flat_params(self, pdev):
        """Device-resident fast path: every parameter's storage IS a slice of one flat fp32 buffer in state_dict order (the layout the
        C-ABI takes), so a forward copies nothing.  Parameters therefore live in fp32 on the device whatever the default dtype is (the
        engine's master weights are fp32; optimizers update the views in place; load_state_dict copies into them).  A later
        .to() / .double() un-does this; the next forward re-establishes it."""
        if self._flat_ok and self._flat is not None and self._flat.device == pdev:
            return self._flat
        params = self._params_in_flat_order()
        flat = torch.zeros(self._spec.flat_size(), dtype=torch.float32, device=pdev)
        with torch.no_grad():
            for p, v in zip(params, _fill_flat(flat, self._spec.param_offsets().values(), params)):
                p.data = v
        self._flat, self._flat_ok = flat, True
        self._gflat = self._gviews = self._gpend = None
        self._anchor = torch.zeros((), device=pdev, requires_grad=True)
        return flat

    def _params_in_flat_order(self):
        if self._param_list is None:
            sd = dict(self.named_parameters())
            self._param_list = [sd[k] for k in self._spec.param_offsets().keys()]
        return self._param_list

    def _host_flat(self, pdev, fill):
        """Parameters on the host: their device staging buffer (self._flat, which is NOT their storage: _flat_ok stays False), holding a copy of them when `fill`."""
        if self._flat is None or self._flat.device != pdev or self._flat_ok:
            self._flat, self._flat_ok = torch.zeros(self._spec.flat_size(), dtype=torch.float32, device=pdev), False
        if fill:
            with torch.no_grad():
                _fill_flat(self._flat, self._spec.param_offsets().values(), self._params_in_flat_order())
        return self._flat

    def _param_route(self, pdev, need_grad):
        """How the parameters reach the engine on the two-call route: (flat buffer, _EngineFn route, the parameter tensors autograd sees)."""
        params = self._params_in_flat_order()
        if params[0].device.type == "cuda":
            # parameters on the device: they are (made) views of the flat fp32 buffer -- no copy in, no copy out
            flat = self._flat_params(pdev)
            if not need_grad:
                return flat, None, []
            if _several_processes():      # gradients through autograd: DDP's hooks see them
                return flat, "p", list(params)
            return flat, "fast", [self._anchor]
        # parameters on the host: a device copy per forward (the slow path: lazy-init call, CPU-pinned evaluation)
        flat = self._host_flat(pdev, fill=not need_grad)
        if not need_grad:
            return flat, None, []
        spec = self._spec
        return None, "flat", [_Flatten.apply(spec.flat_size(), pdev, list(spec.param_offsets().values()), *params)]

    def _flat_exchange(self, full, n_flat, windows):
        """ddp.flat_data_parallel: ONE sum-all-reduce of the flat gradient in full[:n_flat] (the spare elements behind it carry this rank's window count: ddp.py).
        Returns what to divide the summed gradient by, or None when no group is set.  The settings are read when a backward runs, not when its forward did:
        ddp.flat_data_parallel set or cleared between the two takes effect in that backward."""
        if self._flat_ddp is None:
            return None
        from .ddp import exchange_flat_gradient_
        return exchange_flat_gradient_(full, n_flat, windows, None if self._flat_ddp is True else self._flat_ddp, self._flat_ddp_weighted, getattr(self, "_flat_ddp_live", None))

    # ---- construction helpers ---------------------------------------------------------------------
    def _build_convs(self, mean_rels):
        self.encoder = pnn.HeteroDictLinear(-1, self.hidden_channels, self._node_types)
        self.convs = nn.ModuleList()
        h = self.hidden_channels
        for _ in range(self.num_layers):
            conv_dict = {}
            for et in self._edge_types:
                conv_dict[et] = pnn.GraphConv(h, h, aggr="mean" if et[1] in mean_rels else "add")
            self.convs.append(pnn.HeteroConv(conv_dict, aggr="sum"))

    def set_precision(self, dtype: str):
        """"x3" / "f32" / "bf16": the plan of the fused engine (fp32 master parameters in one flat buffer).
        "f64": the reference's own precision (torch.set_default_dtype(torch.float64), gnnLightning.py:1183).  The parameters become fp64 (`self.double()`: a
        load_state_dict of a reference checkpoint then keeps every bit) and no engine is compiled: forward() is `_forward_operators` under
        `ops.compute_dtype("f64")` -- every Linear / GraphConv on the fp64 MFMA operators of csrc/mshgnn_ops.hip, with the model's own activation module,
        autograd for the parameter and the input gradients.  fp64 inputs are read as they are, other dtypes are widened; the output is fp64.  The one-call
        and series routes (`fused_training_step`, `fused_training_step_windows`, `forward_windows`) return None, so their callers assemble and call forward().
        Leaving "f64" calls `self.float()`: the parameters are rounded to fp32 ONCE (f64 -> x3 is not a round trip for parameters that were loaded or trained
        in fp64; x3 -> f64 -> x3 without an update in between is, fp32 -> fp64 being exact), and the next forward re-establishes the flat fp32 buffer."""
        if dtype not in ("f32", "bf16", "x3", "f64"):
            raise ValueError("precision must be 'f32', 'bf16', 'x3' or 'f64'")
        was = self._precision
        self._precision = dtype
        if dtype == "f64":
            self.double()
        elif was == "f64":
            self.float()
        return self

    def set_regression_loss(self, kind: str, delta: float = 1.0):
        """What a regression model trains on: "mse" (the default, the reference's), "l1" or "huber" with `delta` -- torch.nn.MSELoss / L1Loss / HuberLoss(delta).
        Every fused route of the model (`fused_training_step`, `fused_training_step_windows`, the engines' `*_mse*` calls) then computes it; at precision "f64"
        there is no engine and the kind is kept here for the wrappers' fp64 loss.  ValueError on a classification model."""
        from .engine import reg_loss_code
        if not self.regression:
            raise ValueError("set_regression_loss: this is a classification model (cross entropy)")
        reg_loss_code(kind, delta)
        self._reg_loss = (kind, float(delta) if kind == "huber" else 1.0)
        for e in self._engines.values():
            e.set_regression_loss(*self._reg_loss)
        return self

    @property
    def regression_loss(self) -> Tuple[str, float]:
        return getattr(self, "_reg_loss", ("mse", 1.0))

    def _adopt_env_precision(self):
        """MSHGNN_DTYPE=f64 at construction: the parameters exist now, make them fp64 (before any load_state_dict)."""
        if self._precision == "f64":
            self.double()

    def _fused_ok(self) -> bool:
        """The fused engines serve this model: nn.ReLU() and a precision they have a plan for ("f64" has none)."""
        return self._fused_activation and self._precision != "f64"

    def _operator_mode(self):
        """The compute dtype of the operator route: fp64 operators for "f64", else whatever the caller has set (the default: fp32)."""
        import contextlib
        from . import ops
        return ops.compute_dtype("f64") if self._precision == "f64" else contextlib.nullcontext()

    def reset_parameters(self):
        """Reset all learnable parameters (hgnn_c2.py:286-293)."""
        self.encoder.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        if hasattr(self, "base_transform"):
            self.base_transform[0].reset_parameters()
            self.base_transform[2].reset_parameters()
        self.decoder.reset_parameters()

    # ---- plan ---------------------------------------------------------------------------------------
    def _num_nodes(self, x_dict) -> Tuple[int, Dict[str, int]]:
        nb = self.num_bases
        if x_dict["base"].shape[0] % nb:
            raise ValueError(f"x_dict['base'] has {x_dict['base'].shape[0]} rows, not a multiple of {nb} base nodes")
        B = x_dict["base"].shape[0] // nb
        nn_ = {}
        for t in self._node_types:
            if x_dict[t].shape[0] % B:
                raise ValueError(f"x_dict['{t}'] rows ({x_dict[t].shape[0]}) are not a multiple of the batch size {B}")
            nn_[t] = x_dict[t].shape[0] // B
        return B, nn_

    def _make_spec(self, x_dict, edge_index_dict) -> ModelSpec:
        B, nn_ = self._num_nodes(x_dict)
        rels = []
        for et in self._edge_types:
            if et not in edge_index_dict:
                raise ValueError(f"edge_index_dict lacks relation {et} named in data_metadata")
            s, _, d = et
            rels.append((et, infer_window_edges(edge_index_dict[et], nn_[s], nn_[d], B)))
        topo = RobotTopology(name="from-batch", num_nodes={t: nn_[t] for t in NODE_TYPES if t in nn_}, relations=rels)
        widths = {t: int(x_dict[t].shape[1]) for t in self._node_types}
        return ModelSpec(kind=self.kind, topology=topo, hidden=self.hidden_channels, num_layers=self.num_layers,
                         widths=widths, regression=self.regression, grf_dimension=getattr(self, "grf_dimension", 1),
                         group=self._group, num_timesteps=getattr(self, "num_timesteps", 150),
                         com_dimension=getattr(self, "num_dimensions_per_base", 6) if self.kind == "s4_com" else 6)

    def _engine(self, device):
        from .engine import make_engine
        key = (self._precision, str(device))
        if key not in self._engines:
            self._engines[key] = make_engine(self._spec, dtype=self._precision, device=device)
            if self.regression_loss[0] != "mse":
                self._engines[key].set_regression_loss(*self.regression_loss)
        return self._engines[key]

    # ---- forward --------------------------------------------------------------------------------------
    def _prepare(self, x_dict, edge_index_dict):
        """Checks, lazy initialisation and the engine for this call: (spec, B, engine | None, device of the parameters' engine copy)."""
        for t in self._node_types:
            if t not in x_dict:
                raise KeyError(f"x_dict lacks node type '{t}'")
        first = self._spec is None
        if first:
            for t in self._node_types:
                self.encoder.lins[t].materialize(int(x_dict[t].shape[1]))
                lin = self.encoder.lins[t]
                ref = self.decoder.weight
                lin.to(device=ref.device, dtype=ref.dtype)
            self._spec = self._make_spec(x_dict, edge_index_dict)
            expect = list(self._spec.param_shapes().keys())
            have = [k for k, _ in self.named_parameters()]
            if expect != have:
                raise RuntimeError(f"parameter layout mismatch: {set(expect) ^ set(have)}")
        spec = self._spec
        B, nn_ = self._num_nodes(x_dict)
        def _pitch_ok(x, F):     # the reference's width, or rows already at an engine pitch (on-device window assembly): whole 16-byte chunks >= F
            return x.shape[1] == F or (x.dtype in (torch.bfloat16, torch.float32) and x.shape[1] in accepted_pitches(F, x.element_size()))
        for t in self._node_types:
            if nn_[t] != spec.num_nodes[t] or not _pitch_ok(x_dict[t], spec.widths[t]):
                raise ValueError(f"x_dict['{t}'] does not match the compiled topology "
                                 f"({nn_[t]} nodes x {x_dict[t].shape[1]} vs {spec.num_nodes[t]} x {spec.widths[t]})")
        self._check_edges(edge_index_dict, B)
        if not self._fused_ok():
            return spec, B, None, None
        pdev = self.decoder.weight.device
        if pdev.type != "cuda":
            # parameters still on the host (e.g. the wrapper's lazy-init call, gnnLightning.py:593-595, or
            # evaluate_model's model.to('cpu'), :1029): the arithmetic STILL runs in the HIP engine, on the current
            # device, with a device copy of the parameters.  No GPU -> error; there is no CPU implementation.
            if not torch.cuda.is_available():
                raise RuntimeError("the MS-HGNN engine needs a HIP device; there is no CPU fallback")
            pdev = torch.device("cuda", torch.cuda.current_device())
        return spec, B, self._engine(pdev), pdev

    def _check_edges(self, edge_index_dict, B):
        """One host-side check per batch size: the batch is B copies of the compiled graph."""
        if B in self._checked_batches:
            return
        spec = self._spec
        for et in self._edge_types:
            s, _, d = et
            if infer_window_edges(edge_index_dict[et], spec.num_nodes[s], spec.num_nodes[d], B) != spec.topology.edges(et):
                raise ValueError(f"edge_index_dict[{et}] differs from the topology this model was compiled for")
        self._checked_batches.add(B)

    def _shape_output(self, out, spec, B, in_dev, in_dtype):
        out = out.to(device=in_dev, dtype=in_dtype if in_dtype in (torch.float64, torch.float32) else torch.float32)
        return self._view_output(out, spec, B)

    @staticmethod
    def _view_output(out, spec, B):
        if spec.output_is_window_major:
            return out.view(B, -1)      # ms_foot_decoder: [B, 4*3]   (hgnn_c2.py:184-189)
        if spec.kind in ("k4_com", "c2_com"):
            return out.view(B, spec.num_nodes["base"], spec.out_channels)   # morphological_symmetry_decoder, hgnn_k4_com.py:157-165
        return out                      # [B*4, out_channels_per_foot]  (COM S4 / COM_HGNN: [B, com_dimension])

    def fused_training_step(self, x_dict, edge_index_dict, y):
        """forward + the wrapper's loss + backward in ONE engine call (mshgnn_step_mse / mshgnn_step_ce: the decoder, the loss and the decoder's
        backward run in the tail of the fused forward kernel) for a caller that has the labels at forward time -- the training-step wrappers.
        y: the batch's labels (regression: B * n_out * out_channels values; classification: B * 4 contact flags).  Returns (out, loss):
        `out` as forward() returns it (no autograd), `loss` a scalar whose backward() delivers the parameter gradients the engine has
        already computed (times the upstream factor) -- same values as forward() + loss + backward() through autograd.
        Returns None when this route does not apply (gradients disabled, parameters on the host, the operator-by-operator path, more than
        one process without `ddp.flat_data_parallel`: torch's DDP needs the per-parameter autograd hooks); the caller then takes the two-call route."""
        spec, B, e, pdev = self._prepare(x_dict, edge_index_dict)
        params = self._params_in_flat_order()
        if e is None or not torch.is_grad_enabled() or params[0].device.type != "cuda" or not all(p.requires_grad for p in params):
            return None
        if any(x_dict[t].requires_grad for t in self._node_types):      # the caller wants x.grad too: the two-call route (forward() + backward) delivers it
            return None
        if self._flat_ddp is None and _several_processes():
            return None
        in_dev, in_dtype = x_dict[self._node_types[0]].device, x_dict[self._node_types[0]].dtype
        xs = e.cast_inputs(x_dict)
        self._flat_params(pdev)
        if spec.regression:
            target = y.detach().to(pdev, torch.float32).flatten().contiguous()
        else:
            target = (y.detach().to(pdev) != 0).to(torch.int32).flatten().contiguous()
        step = e.step_mse if spec.regression else e.step_ce
        loss, out = _FusedStepFn.apply(self._anchor, self, lambda g: step(xs, self._flat, target, B, grad_flat=g)[:2])
        return self._shape_output(out, spec, B, in_dev, in_dtype), loss

    def fused_training_step_windows(self, batch):
        """`fused_training_step` for a `windows.WindowBatch`: the encoder gathers the batch's inputs straight from the sequence's resident
        series (mshgnn_step_mse_series / mshgnn_step_ce_series, standardised recipes: mshgnn_step_mse_series_std / mshgnn_step_ce_series_std -- no
        separate assembly pass over the windows); the labels (and the materialised windows) are left on the batch.  Returns (out, loss), or None when
        this route does not apply (`_window_route` with training=True is the rule); the caller then assembles the windows and takes `fused_training_step`."""
        e = self._window_route(batch, training=True)
        if e is None:
            return None
        spec, store, B, r = self._spec, batch.store, batch.batch_size, batch.store.recipe
        self._flat_params(store.device)
        if r.normalize:
            step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
        else:
            step = e.step_mse_series if spec.regression else e.step_ce_series

        def run(g):
            xs, y, out, loss, _ = step(store, batch.starts, self._flat, grad_flat=g)
            _, yf, q = store._buffers(B)
            batch._labels_from_step(xs, yf, q)
            return out, loss
        loss, out = _FusedStepFn.apply(self._anchor, self, run)
        return self._shape_output(out, spec, B, store.device, torch.float32), loss

    def forward_windows(self, batch):
        """The evaluation forward for a `windows.WindowBatch` without autograd: the encoder gathers the batch's inputs straight from the sequence's
        resident series (mshgnn_forward_series -- no assembly pass, no materialised windows; standardised recipes included) and the labels are left
        on the batch.  Returns the output as forward() does -- bit-identical to forward(batch.x_dict, ...) -- or None when this route does not
        apply (`_window_route` with training=False is the rule); the caller then assembles the windows and calls forward()."""
        e = self._window_route(batch, training=False)
        if e is None:
            return None
        spec, store, B = self._spec, batch.store, batch.batch_size
        y, q, _, out = e.forward_series(store, batch.starts, self._flat_params(store.device))
        if y is not None:
            batch._labels_from_step(None, y, q)
        return self._shape_output(out, spec, B, store.device, torch.float32)

    def _window_route(self, batch, training):
        """The engine for `fused_training_step_windows` (training) or `forward_windows` (evaluation) on this batch, or None when the batch takes the assembled
        route instead.  Cheap checks first (_window_recipe_ok), then the parameters' device and the grad mode; the engine is looked up only after those pass."""
        store, r = batch.store, batch.store.recipe
        if not self._fused_ok() or not _window_recipe_ok(self._spec, r, store.desc, store.dtype, training):
            return None
        params = self._params_in_flat_order()
        if params[0].device.type != "cuda" or params[0].device != store.device or torch.is_grad_enabled() != training:
            return None
        if training:
            # fused_training_step's own conditions: torch's DDP needs the per-parameter autograd hooks, and a frozen parameter needs the two-call route
            if not all(p.requires_grad for p in params) or (self._flat_ddp is None and _several_processes()):
                return None
        e = self._engine(store.device)
        if e.generic or e.storage not in ("bf16", "x3") or (e.storage == "bf16") != (store.dtype == "bf16"):      # (the split plan gathers fp32 series)
            return None
        if training and getattr(e, "padded", False):      # engine.PaddedEngine has no series steps (its forward_series pads the parameters itself)
            return None
        if not training:
            if not hasattr(e.lib, "mshgnn_forward_series"):
                return None
            # evaluation leaves labels on the batch only when the recipe has some, and then they must be the model's targets (training: the library's step checks them)
            if r.label_cols and len(r.label_cols) != e.n_out * (self._spec.out_channels if self._spec.regression else 1):
                return None
        self._check_edges(batch.edge_index_dict, batch.batch_size)
        return e

    def forward(self, x_dict, edge_index_dict):
        spec, B, e, pdev = self._prepare(x_dict, edge_index_dict)
        if e is None:
            with self._operator_mode():
                return self._forward_operators(x_dict, edge_index_dict, B)
        in_dev, in_dtype = x_dict[self._node_types[0]].device, x_dict[self._node_types[0]].dtype
        xs = e.cast_inputs(x_dict)
        grad_on = torch.is_grad_enabled()
        need_grad = grad_on and any(p.requires_grad for p in self._params_in_flat_order())
        # the caller's tensors enter autograd only when one of them wants its gradient (_EngineFn)
        xin = [x_dict[t] for t in self._node_types] if grad_on and any(x_dict[t].requires_grad for t in self._node_types) else []
        flat, route, ptens = self._param_route(pdev, need_grad)
        if route is None and not xin:
            with torch.no_grad():
                out = e.forward(xs, flat, B, training=False)
        else:
            out = _EngineFn.apply((self, e, B, flat, xs, route, len(ptens)), *ptens, *xin)
        return self._shape_output(out, spec, B, in_dev, in_dtype)

    def _forward_operators(self, x_dict, edge_index_dict, B):
        """The reference's forward (hgnn_c2.py:133-182, hgnn_k4.py:146-196, hgnn.py:57-62, hgnn_*_com.py) operator by operator, for models built with
        an activation_fn other than nn.ReLU() and for the "f64" precision: every Linear / GraphConv runs on the HIP operators of ops.py with autograd (in the
        compute dtype forward() sets: fp64 for "f64"), the activation itself is the caller's module.  Inputs and parameters must be on the device."""
        from . import ops
        spec, act = self._spec, self.activation
        dev = x_dict[self._node_types[0]].device
        if dev.type != "cuda":
            raise RuntimeError("the operator path of a non-ReLU model runs on a HIP device (inputs are on the host); there is no CPU fallback")
        wide = self._precision == "f64"
        if self.decoder.weight.device != dev:
            home = self.decoder.weight.device
            if wide and home.type == "cpu" and not torch.is_grad_enabled():
                # "f64", host parameters, no autograd (the wrappers' lazy-initialising call, gnnLightning.py:593-595): as on the engine route the arithmetic
                # still runs on the device, with the parameters there for the duration of the call (a round trip of fp64 tensors: every bit kept)
                self.to(dev)
                try:
                    return self._forward_operators(x_dict, edge_index_dict, B)
                finally:
                    self.to(home)
            raise RuntimeError("move the model to the inputs' device first (model.to(device))")
        x = {}
        for t, m in spec.input_masks().items():                # apply_symmetry (hgnn_c2.py:191-284) as its net +-1 masks
            v = x_dict[t]
            if wide:      # "f64": fp64 inputs as they are, anything else widened (exact); rows at an engine pitch (a windows.WindowBatch: _prepare checked it) lose their pad columns
                v = v[:, :spec.widths[t]].to(torch.float64)
            if v.shape[1] != spec.widths[t]:
                raise ValueError(f"x_dict['{t}'] must have the reference's width {spec.widths[t]} on the operator path")
            n = m.shape[0]
            x[t] = (v.view(-1, n, v.shape[1]) * m.to(v.device, v.dtype).unsqueeze(0)).reshape(v.shape)
        x = {k: act(v) for k, v in self.encoder(x).items()}
        bt = getattr(self, "base_transform", None)
        for conv in self.convs:
            h = conv(x, edge_index_dict)
            if spec.kind in ("mi", "s4_com") or bt is None:
                x = {k: act(v) for k, v in h.items()}
                continue
            new = {}
            for k, v in h.items():
                if k == "base":                                   # base_transform: Linear, nn.ReLU() (fixed in the reference), Linear
                    new[k] = ops.linear(torch.relu(ops.linear(v, bt[0].weight, bt[0].bias)), bt[2].weight, bt[2].bias)
                else:
                    new[k] = act(v)
            x = {k: new[k] + x[k] if (k in x and x[k].shape == new[k].shape) else new[k] for k in new}
        out = self.decoder(x[spec.out_type])
        n_out = spec.num_nodes[spec.out_type]
        out = (out.view(B, n_out, -1) * spec.output_mask().to(out.device, out.dtype).unsqueeze(0)).reshape(B * n_out, -1)
        return self._view_output(out, spec, B)

    # ---- reference helper kept for API compatibility ------------------------------------------------------
    def apply_symmetry(self, x_dict):
        """Elementwise +-1 masks equivalent to the reference's apply_symmetry (hgnn_c2.py:191-231).  The engine
        folds these into its encoder loads; this method exists for callers that use it directly."""
        spec = self._spec if self._spec is not None else self._make_spec(x_dict, {})
        masks = spec.input_masks()
        for t, m in masks.items():
            x = x_dict[t]
            n = m.shape[0]
            x_dict[t] = (x.view(-1, n, x.shape[1]) * m.to(x.device, x.dtype).unsqueeze(0)).reshape(x.shape)
        return x_dict


class _SymmetryHelpers:
    """The tensor helpers the reference's C2 / K4 models carry next to `apply_symmetry` (hgnn_c2.py:184-189, 233-284; hgnn_k4.py): the engine needs
    none of them (the masks are sign-bit XORs inside its encoder, the output mask sits in its decoder tail), they exist for callers that use them."""

    def ms_foot_decoder(self, x):
        """[B * num_legs, out_channels_per_foot] decoder rows -> [B, num_legs * out_channels_per_foot] times the feet's +-1 mask (hgnn_c2.py:184-189)."""
        x = x.view(-1, self.num_legs, self.out_channels_per_foot).flatten(start_dim=1)
        return self.feet_linear_weights.to(x.device) * x

    def unpack_data(self, data, batch_size, num_nodes):
        """Node rows [batch * nodes, 2 * dims * T] laid out [variable][axis][time] -> the two variables as [batch, T, nodes * dims]
        (hgnn_c2.py:233-264)."""
        d, t = self.num_dimensions_per_foot, self.num_timesteps
        x = data.view(batch_size, num_nodes, 2, d, t).permute(2, 0, 4, 1, 3)           # [variable, batch, time, node, axis]
        return x[0].reshape(batch_size, t, num_nodes * d), x[1].reshape(batch_size, t, num_nodes * d)

    def pack_data(self, f_p, f_v, batch_size, num_nodes):
        """The inverse of `unpack_data` (hgnn_c2.py:266-284)."""
        d, t = self.num_dimensions_per_foot, self.num_timesteps
        both = torch.stack([f_p.view(batch_size, t, num_nodes, d), f_v.view(batch_size, t, num_nodes, d)])      # [variable, batch, time, node, axis]
        return both.permute(1, 3, 0, 4, 2).reshape(batch_size * num_nodes, 2 * d * t)


def _load_group(symmetry_mode, group_operator_path):
    if symmetry_mode and group_operator_path:
        with open(group_operator_path, "r") as f:
            return yaml.safe_load(f)
    return None


class GRF_HGNN_C2(_SymmetryHelpers, _MSHGNNBase):
    """MS-HGNN for the C2 graph (2 base nodes) -- drop-in for hgnn_c2.py:GRF_HGNN_C2."""
    kind = "c2"
    num_bases = 2

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), symmetry_mode: str = None, group_operator_path: str = None,
                 grf_dimension: int = 3):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.num_timesteps = 150           # hard-coded in the reference (hgnn_c2.py:30)
        self.num_legs = 4
        self.num_joints = 12
        self.num_dimensions_per_foot = 3
        self.num_dimensions_per_base = 3
        self.num_variables_per_joint = 3 if regression else 2
        self.grf_dimension = grf_dimension
        self._group = _load_group(symmetry_mode, group_operator_path)
        self._build_convs(mean_rels=("center_bb",))
        h = hidden_channels
        self.base_transform = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        if regression and grf_dimension == 1:
            self.out_channels_per_foot = 1
        elif regression and grf_dimension == 3:
            self.out_channels_per_foot = 3
        else:
            self.out_channels_per_foot = 2
        self.decoder = pnn.Linear(h, self.out_channels_per_foot)
        coeffs = ModelSpec.symmetry_coefficients(self._coeff_probe())
        self.joints_linear_weights, self.feet_linear_weights, self.base_coefficients_lin, self.base_coefficients_ang = coeffs
        self._adopt_env_precision()

    def _coeff_probe(self):
        class _P:  # minimal duck-type for ModelSpec.symmetry_coefficients
            pass
        p = _P()
        p.kind, p.group, p.num_nodes = self.kind, self._group, {"base": self.num_bases}
        return p


class GRF_HGNN_K4(_SymmetryHelpers, _MSHGNNBase):
    """MS-HGNN for the K4 graph (4 base nodes) -- drop-in for hgnn_k4.py:GRF_HGNN_K4."""
    kind = "k4"
    num_bases = 4

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), symmetry_mode: str = None, group_operator_path: str = None):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.num_timesteps = 150           # hgnn_k4.py:29
        self.num_legs = 4
        self.num_joints = 12
        self.num_dimensions_per_foot = 3
        self.num_dimensions_per_base = 3
        self._group = _load_group(symmetry_mode, group_operator_path)
        self._build_convs(mean_rels=("gt", "gs"))
        h = hidden_channels
        self.base_transform = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        self.out_channels_per_foot = 1 if regression else 2
        self.decoder = pnn.Linear(h, self.out_channels_per_foot)
        coeffs = ModelSpec.symmetry_coefficients(GRF_HGNN_C2._coeff_probe(self))
        self.joints_linear_weights, self.feet_linear_weights, self.base_coefficients_lin, self.base_coefficients_ang = coeffs
        self._adopt_env_precision()


class GRF_HGNN(_MSHGNNBase):
    """MI-HGNN baseline (1 base node, no masks / base MLP / residual) -- drop-in for hgnn.py:GRF_HGNN."""
    kind = "mi"
    num_bases = 1

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), grf_dimension: int = 1):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.grf_dimension = grf_dimension
        self._build_convs(mean_rels=())
        if regression and grf_dimension == 1:
            self.out_channels_per_foot = 1
        elif regression and grf_dimension == 3:
            self.out_channels_per_foot = 3
        else:
            self.out_channels_per_foot = 2
        self.decoder = pnn.Linear(hidden_channels, self.out_channels_per_foot)
        self._adopt_env_precision()


class _COMSymBase(_MSHGNNBase):
    """Shared constructor of the Solo centroidal-momentum MS-HGNNs: joints carry (q, qd) of one time step, the decoder
    reads the base nodes and emits [lin(3) | ang(3)] per base node (hgnn_k4_com.py:22-123, hgnn_c2_com.py:22-108)."""
    _mean_rels = ("gt", "gs")

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), symmetry_mode: str = None, group_operator_path: str = None):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.num_timesteps = 1             # hgnn_k4_com.py:29
        self.num_legs = 4
        self.num_joints = 12
        self.num_dimensions_per_base = 6
        self._group = _load_group(symmetry_mode, group_operator_path)
        self._build_convs(mean_rels=self._mean_rels)
        h = hidden_channels
        self.base_transform = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        self.decoder = pnn.Linear(h, self.num_dimensions_per_base)
        coeffs = ModelSpec.symmetry_coefficients(GRF_HGNN_C2._coeff_probe(self))
        self.joints_linear_weights, _, self.base_coefficients_lin, self.base_coefficients_ang = coeffs
        self._adopt_env_precision()

    def morphological_symmetry_decoder(self, x):
        """The reference's output mask as a standalone helper (hgnn_k4_com.py:157-165); forward() already applies it
        inside the decoder kernel."""
        nb = self.num_bases
        x = x.reshape(-1, nb, 6)
        m = torch.cat((self.base_coefficients_lin.view(nb, 3), self.base_coefficients_ang.view(nb, 3)), dim=1)
        return x * m.to(x.device, x.dtype).unsqueeze(0)


class COM_HGNN_K4(_COMSymBase):
    """Centroidal-momentum MS-HGNN on the Solo K4 graph (4 base nodes) -- drop-in for hgnn_k4_com.py:COM_HGNN_K4."""
    kind = "k4_com"
    num_bases = 4


class COM_HGNN_C2(_COMSymBase):
    """Centroidal-momentum MS-HGNN on the Solo C2 graph (2 base nodes) -- drop-in for hgnn_c2_com.py:COM_HGNN_C2."""
    kind = "c2_com"
    num_bases = 2


class COM_HGNN_S4(_MSHGNNBase):
    """Centroidal-momentum baseline on the single-base graph (no masks / base MLP / residual) -- drop-in for
    hgnn_s4_com.py:COM_HGNN_S4.  symmetry_mode / group_operator_path are accepted and unused, as in the reference."""
    kind = "s4_com"
    num_bases = 1

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), symmetry_mode: str = None, group_operator_path: str = None):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.num_legs = 4
        self.num_joints = 12
        self.num_dimensions_per_base = 6
        self._build_convs(mean_rels=())
        self.decoder = pnn.Linear(hidden_channels, self.num_dimensions_per_base)
        self._adopt_env_precision()


class COM_HGNN(_MSHGNNBase):
    """MI-HGNN with the decoder on the base node -- drop-in for hgnn.py:COM_HGNN (hgnn.py:66-117)."""
    kind = "s4_com"
    num_bases = 1

    def __init__(self, hidden_channels: int, num_layers: int, data_metadata, regression: bool = True,
                 activation_fn=nn.ReLU(), com_dimension: int = 6):
        super().__init__()
        self._init_common(hidden_channels, num_layers, data_metadata, regression, activation_fn)
        self.num_dimensions_per_base = com_dimension
        self._build_convs(mean_rels=())
        self.decoder = pnn.Linear(hidden_channels, self.num_dimensions_per_base)
        self._adopt_env_precision()


# ---- the MLP baseline (gnnLightning.py:363-413, gnnLightning_com.py:234-287) ---------------------------------------------------------------------------
class _MLPSpec:
    """What the module surface (the flat-parameter views, _FusedStepFn, _deliver_gradients, the flat optimizers) reads of a model's spec, for the MLP: the
    flat layout in torch's state_dict order of the reference's nn.Sequential, one window = one row."""

    def __init__(self, in_channels, hidden, out_channels, num_layers, regression):
        self.in_channels, self.hidden, self.out_channels, self.num_layers, self.regression = in_channels, hidden, out_channels, num_layers, regression
        self.node_types, self.num_nodes, self.out_type = ["mlp"], {"mlp": 1}, "mlp"
        self._offsets, self._shapes, o = {}, {}, 0
        for i in range(num_layers):
            of, kf = (hidden if i < num_layers - 1 else out_channels), (in_channels if i == 0 else hidden)
            self._offsets[f"{2 * i}.weight"], self._shapes[f"{2 * i}.weight"] = (o, of * kf), (of, kf); o += of * kf
            self._offsets[f"{2 * i}.bias"], self._shapes[f"{2 * i}.bias"] = (o, of), (of,); o += of
        self._n = o

    def param_offsets(self):
        return self._offsets

    def param_shapes(self):
        return self._shapes

    def flat_size(self):
        return self._n


class _MLPFn(torch.autograd.Function):
    """The two-call route of MLP.forward on the fused engine: engine.forward(training) here, mshgnn_mlp_backward in backward.  cfg: (model, engine, flat, rows,
    route, number of parameter tensors); the parameters travel by `route` exactly as in _EngineFn.  No gradient with respect to the inputs."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        model, e, flat, xs, route, n_p = cfg
        if route == "flat":
            flat = tensors[0]
        out = e.forward(xs, flat, training=True)
        model._fwd_id += 1
        ctx.cfg, ctx.flat, ctx.ticket = cfg, flat, model._fwd_id
        ctx.shapes = [p.shape for p in tensors[:n_p]]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        model, e, _, xs, route, n_p = ctx.cfg
        flat = ctx.flat
        if model._fwd_id != ctx.ticket:
            raise RuntimeError("the activation stash of this forward was overwritten by a later forward of the same model; call backward before the next forward")
        g32 = gout.contiguous().to(torch.float32)
        if route == "fast":
            _deliver_gradients(model, flat, lambda target: e.backward(xs, flat, g32, grad_flat=target))
            return (None, None)
        if route == "flat":
            return (None, e.backward(xs, flat, g32))
        gflat = e.backward(xs, flat, g32)
        return (None, *[gflat[o:o + n].view(shape) for (o, n), shape in zip(model._spec.param_offsets().values(), ctx.shapes)])


class MLP(_MSHGNNBase):
    """The reference's MLP baseline as a module: `num_layers` nn.Linear layers with the activation between them, created by torch's own nn.Linear in the
    reference's order under the reference's names (state_dict keys 0.weight, 0.bias, 2.weight, ...: the same seed gives the same initial weights as
    nn.Sequential(*modules), gnnLightning.py:391-407).  forward(x [B, in_channels]) -> [B, out_channels] routes by the module surface's one rule:
      precision "x3" (the default: the split-bf16 parity plan, 1e-4 of fp64) or "bf16", nn.ReLU(), a shape the fused engine takes, parameters on the device
        -> the engine.MLPEngine of that precision through one autograd.Function;
      anything else on a HIP device (set_precision("f32"), another activation, another width) -> operator by operator on ops.linear (fp32 MFMA).
    There is no CPU path."""
    kind = "mlp"
    num_bases = 1
    num_dimensions_per_base = 6

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int, activation_fn=nn.ReLU(), regression: bool = True):
        super().__init__()
        if num_layers < 2:
            raise ValueError("num_layers must be 2 or greater")
        self._init_common(hidden_channels, num_layers, (["mlp"], []), regression, activation_fn)
        self.in_channels, self.out_channels = in_channels, out_channels
        dims = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        for i in range(num_layers):
            self.add_module(str(2 * i), nn.Linear(dims[i], dims[i + 1]))
            if i < num_layers - 1:
                self.add_module(str(2 * i + 1), activation_fn)
        self._spec = _MLPSpec(in_channels, hidden_channels, out_channels, num_layers, regression)
        self._fwd_id = 0
        self._adopt_env_precision()

    def linears(self):
        return [getattr(self, str(2 * i)) for i in range(self.num_layers)]

    def __len__(self):
        return 2 * self.num_layers - 1

    def __getitem__(self, i):
        return getattr(self, str(range(len(self))[i]))

    def _fused(self) -> bool:
        from . import engine as eng
        return (self._fused_activation and self._precision in ("bf16", "x3")
                and eng.mlp_supported(self.in_channels, self.hidden_channels, self.out_channels, self.num_layers))

    def _engine(self, device):
        from . import engine as eng
        key = (self._precision, str(device))
        if key not in self._engines:
            self._engines[key] = eng.MLPEngine(self.in_channels, self.hidden_channels, self.out_channels, self.num_layers, self._precision, device)
            if self.regression_loss[0] != "mse":
                self._engines[key].set_regression_loss(*self.regression_loss)
        return self._engines[key]

    def _device_of(self, x):
        p = self._params_in_flat_order()[0]
        dev = p.device if p.device.type == "cuda" else x.device
        if dev.type != "cuda":
            raise RuntimeError("the MLP runs on a HIP device (parameters and inputs are on the host); there is no CPU fallback")
        return dev

    def forward(self, x):
        x2 = x.reshape(-1, self.in_channels) if x.dim() != 2 else x
        dev = self._device_of(x2)
        if not self._fused():
            return self._forward_operators_mlp(x2, dev)
        e = self._engine(dev)
        xs = e.cast_input(x2.detach())
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self._params_in_flat_order())
        flat, route, ptens = self._param_route(dev, need_grad)
        if route is None:
            with torch.no_grad():
                out = e.forward(xs, flat, training=False)
        else:
            out = _MLPFn.apply((self, e, flat, xs, route, len(ptens)), *ptens)
        return out.to(x.dtype) if x.dtype in (torch.float64, torch.float32) and out.dtype != x.dtype else out

    def _forward_operators_mlp(self, x, dev):
        """Operator by operator on ops.linear (fp32 MFMA, autograd through ops._Linear): the parity route.  Precision "f64": the same on the fp64 MFMA
        operators, without the casts -- fp64 parameters, inputs widened to fp64, an fp64 output."""
        from . import ops
        lin = self.linears()
        if lin[0].weight.device != dev:
            raise RuntimeError("move the model to the inputs' device first (model.to(device))")
        dt = torch.float64 if self._precision == "f64" else torch.float32
        a = x.to(dev, dt)
        with self._operator_mode():
            for i, m in enumerate(lin):
                a = ops.linear(a, m.weight.to(dt), m.bias.to(dt))
                if i < len(lin) - 1:
                    a = self.activation(a)
        return a

    # ---- the one-call routes of the wrappers on a windows.WindowBatch ----
    def _window_route(self, batch, training):
        store, r = batch.store, batch.store.recipe
        if not self._fused() or len(r.node_types) != 1 or r.num_nodes[r.node_types[0]] != 1 or r.width(r.node_types[0]) != self.in_channels:
            return None
        params = self._params_in_flat_order()
        if params[0].device.type != "cuda" or params[0].device != store.device or torch.is_grad_enabled() != training:
            return None
        n_target = self.out_channels if self.regression else self.out_channels // 2
        if training:
            if not all(p.requires_grad for p in params) or _several_processes() or len(r.label_cols) != n_target or (not self.regression and self.out_channels % 2):
                return None
        elif r.label_cols and len(r.label_cols) != n_target:
            return None
        return self._engine(store.device)

    def _leave_labels(self, e, batch):
        store, B = batch.store, batch.batch_size
        if e._series_ok(store):
            y, q, _, _ = store.eval_buffers(B, True, self.out_channels // 2 if (not self.regression and self.out_channels % 2 == 0) else 0)
        else:
            _, y, q = store._buffers(B)
        batch._labels_from_step(None, y, q)

    def fused_training_step_windows(self, batch):
        """forward + the wrapper's loss + backward for a `windows.WindowBatch` as ONE MLPEngine.step_*_series call (the rows gathered from the resident series);
        the labels are left on the batch.  Returns (out, loss) as _MSHGNNBase.fused_training_step_windows does, or None when the route does not apply."""
        e = self._window_route(batch, training=True)
        if e is None:
            return None
        store = batch.store
        self._flat_params(store.device)
        step = e.step_mse_series if self.regression else e.step_ce_series

        def run(g):
            _, out, loss, _ = step(store, batch.starts, self._flat, grad_flat=g)
            self._leave_labels(e, batch)
            return out, loss
        loss, out = _FusedStepFn.apply(self._anchor, self, run)
        return out, loss

    def forward_windows(self, batch):
        """The evaluation forward for a `windows.WindowBatch` without autograd (MLPEngine.forward_series); None when the route does not apply."""
        e = self._window_route(batch, training=False)
        if e is None:
            return None
        y, q, _, out = e.forward_series(batch.store, batch.starts, self._flat_params(batch.store.device), labels=bool(batch.store.recipe.label_cols))
        if y is not None:
            batch._labels_from_step(None, y, q)
        return out

    def fused_training_step(self, x, y):
        """The one-call step on the caller's own rows ((x, y) tuple batches): (out, loss) or None."""
        params = self._params_in_flat_order()
        if not self._fused() or not torch.is_grad_enabled() or params[0].device.type != "cuda" or not all(p.requires_grad for p in params) or _several_processes():
            return None
        dev = params[0].device
        e = self._engine(dev)
        xs = e.cast_input(x.reshape(-1, self.in_channels).detach())
        B = xs.shape[0]
        self._flat_params(dev)
        if self.regression:
            target, step = y.detach().to(dev, torch.float32).reshape(B, self.out_channels).contiguous(), e.step_mse
        else:
            target, step = (y.detach().to(dev) != 0).to(torch.int32).reshape(B, self.out_channels // 2).contiguous(), e.step_ce
        loss, out = _FusedStepFn.apply(self._anchor, self, lambda g: step(xs, self._flat, target, grad_flat=g)[:2])
        return out, loss

    def reset_parameters(self):
        for m in self.linears():
            m.reset_parameters()
