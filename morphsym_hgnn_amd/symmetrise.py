"""Symmetrisation: a model's predictions averaged over the orbit of a morphological symmetry group,

    f_sym(x) = 1/|G| . sum_g rho_out(g)^-1 f(rho_in(g) x),

which makes ANY model exactly equivariant -- the third way to a symmetric model next to an equivariant architecture (the MS-HGNN families) and augmentation
over the orbit (`store.orbit(group)` as a training set).  The reference has no such layer; it is the baseline its tables lack next to MI-HGNN and the MLP.

An ORBIT-COMPLETE batch (`SequenceStore.orbit_batch`, `DatasetView.orbit_batch`) holds K . B windows element-major: window e . B + w is element e of base window
w.  The OUTPUT ACTION of element e (`OutputAction`) is a permutation with signs over the output's units, y_e[k] = sign[e][k] . y[perm[e][k]] -- the label tables
of the orbit store's element recipes, which the reference's own dataset classes pin.  The device side is three launches of csrc/mshgnn_orbit.hip
(include/mshgnn.h has the contract): `orbit_average` (an autograd function over the average and its exact transpose), `EquivarianceDefect` (how far the raw
model is from equivariant, per operator) -- both deterministic, no floating-point atomic.  `Symmetrised(wrapper, action)` runs a wrapper's steps on the averaged
prediction; `evaluate_sequence_symmetrised` sweeps a sequence.  No CPU implementation: without the library's kernels these raise.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import engine as eng

MAX_ELEMENTS, MAX_UNITS, MAX_WIDTH = 8, 64, 16      # MSHGNN_WINDOW_MAX_ELEMENTS and the limits of mshgnn_orbit_* (include/mshgnn.h)


class OutputAction:
    """How the K elements of an orbit act on a model's output: host tables perm[e][k], sign[e][k] in {+1, -1} over `n_units` units of `width` consecutive
    floats, y_e[k] = sign[e][k] . y[perm[e][k]]; element 0 is the identity.  Regression: n_units = n_out . out_channels, width 1; classification: n_units =
    n_out feet, width 2 (the logit pair), all signs +1.  `operators` names the elements (None: the identity)."""

    def __init__(self, perm, sign, width: int, operators: Optional[Sequence] = None):
        perm = [[int(x) for x in row] for row in perm]
        sign = [[int(x) for x in row] for row in sign]
        K = len(perm)
        if not 1 <= K <= MAX_ELEMENTS or len(sign) != K:
            raise ValueError(f"an output action has 1 to {MAX_ELEMENTS} elements with one perm and one sign row each, not {K} / {len(sign)}")
        U = len(perm[0])
        if not 1 <= U <= MAX_UNITS:
            raise ValueError(f"n_units must be in [1, {MAX_UNITS}], not {U}")
        if not 1 <= int(width) <= MAX_WIDTH:
            raise ValueError(f"width must be in [1, {MAX_WIDTH}], not {width}")
        for e in range(K):
            if len(perm[e]) != U or len(sign[e]) != U or sorted(perm[e]) != list(range(U)):
                raise ValueError(f"element {e}: perm is not a permutation of [0, {U})")
            if any(c not in (-1, 1) for c in sign[e]):
                raise ValueError(f"element {e}: signs must be +-1")
        if perm[0] != list(range(U)) or any(c != 1 for c in sign[0]):
            raise ValueError("element 0 must be the identity with sign +1 (an orbit made with identity=True)")
        self.perm, self.sign, self.width = perm, sign, int(width)
        self.n_elements, self.n_units = K, U
        self.operators = list(operators) if operators is not None else [None] + [f"g{e}" for e in range(1, K)]
        if len(self.operators) != K:
            raise ValueError(f"{len(self.operators)} operator names for {K} elements")
        self._perm_c = (C.c_int32 * (K * U))(*[x for row in perm for x in row])
        self._sign_c = (C.c_int32 * (K * U))(*[x for row in sign for x in row])

    @property
    def row(self) -> int:
        """floats of one window's output: n_units . width"""
        return self.n_units * self.width

    @classmethod
    def from_tables(cls, perm, sign, width: int, operators: Optional[Sequence] = None) -> "OutputAction":
        return cls(perm, sign, width, operators)

    @classmethod
    def from_store(cls, orbit_store, regression: bool) -> "OutputAction":
        """The action on the labels of an `orbit` store (or a `DatasetView` of an orbit dataset), read off its element recipes -- not off the group file again:
        perm[e][k] = the position in element 0's `label_cols` of element e's `label_cols[k]`, sign[e][k] = element e's `label_signs[k]` times element 0's at
        that position.  One rule for 3-D GRFs ('fs' tables: 12 units with reflections), 1-D GRFs and contact flags ('ls': 4 units) and the MLP recipes.
        Recipes that all carry `label_slots` (the Solo centroidal-momentum recipes made with symmetry=True, whose label columns repeat once per base node) are read by
        slot instead of by column: 6, 12 or 24 units of width 1.
        ValueError: a store with one element, an orbit made with identity=False, a recipe without labels, duplicate label columns in element 0 without slot
        tracking (the default Solo recipes), a -1 sign with regression=False (logit pairs have no sign to flip)."""
        store = getattr(orbit_store, "dataset", orbit_store)
        recipes = list(getattr(store, "element_recipes", []) or [])
        if int(getattr(store, "n_elements", 1)) < 2 or len(recipes) < 2:
            raise ValueError("OutputAction.from_store needs an `orbit` store: this one has a single group element")
        return cls.from_recipes(recipes, regression, list(store.operators))

    @classmethod
    def from_recipes(cls, recipes, regression: bool, operators: Optional[Sequence] = None) -> "OutputAction":
        """`from_store`'s rule on the element recipes themselves (`WindowRecipe.orbit`), on the host; operators: the elements' names, None = the identity."""
        recipes = list(recipes)
        if len(recipes) < 2:
            raise ValueError("an orbit of one element has nothing to average over")
        ops = list(operators) if operators is not None else [None] + [f"g{e}" for e in range(1, len(recipes))]
        if ops[0] is not None:
            raise ValueError("the orbit was made with identity=False: symmetrisation needs element 0 to be the identity")
        lab0 = [int(c) for c in recipes[0].label_cols]
        if not lab0:
            raise ValueError("the store's recipe has no labels: the output action is read off the label tables")
        slotted = all(getattr(r, "label_slots", None) is not None for r in recipes)
        # recipes that track their label slots (the Solo recipes made with symmetry=True: the 6 columns of Y repeat once per base node) name a label by its
        # slot; every other recipe by its column, which must then be unique
        key0 = [int(s) for s in recipes[0].label_slots] if slotted else lab0
        if len(set(key0)) != len(key0):
            raise ValueError("element 0 has duplicate label columns (the Solo centroidal-momentum recipes without symmetry=True): no permutation can be read off them")
        where = {c: k for k, c in enumerate(key0)}
        sg0 = [int(x) for x in (recipes[0].label_signs or [1] * len(lab0))]
        perm, sign = [], []
        for e, r in enumerate(recipes):
            lab = [int(c) for c in (r.label_slots if slotted else r.label_cols)]
            if sorted(lab) != sorted(key0):
                raise ValueError(f"element {e}: its label {'slots' if slotted else 'columns'} are not a permutation of element 0's")
            sg = [int(x) for x in (r.label_signs or [1] * len(lab))]
            perm.append([where[c] for c in lab])
            sign.append([sg[k] * sg0[perm[e][k]] for k in range(len(lab))])
        if not regression and any(c < 0 for row in sign for c in row):
            raise ValueError("a -1 label sign with regression=False: a classification output (logit pairs) has no sign to flip")
        return cls(perm, sign, 1 if regression else 2, ops)


def _as_rows(out: torch.Tensor, action: OutputAction, windows: int) -> torch.Tensor:
    if not out.is_cuda:
        raise RuntimeError("orbit averaging runs on a HIP device; there is no CPU fallback")
    windows = int(windows)
    if windows < 1 or out.numel() != action.n_elements * windows * action.row:
        raise ValueError(f"an orbit-complete batch of {windows} base windows has {action.n_elements} x {windows} x {action.row} output values, not {out.numel()}")
    return out.detach().contiguous().to(torch.float32).view(action.n_elements * windows, action.row)


def _launch(name: str, action: OutputAction, src: torch.Tensor, windows: int, dst: torch.Tensor) -> None:
    lib = eng.load_library()
    if not hasattr(lib, name):
        raise eng.MshgnnError(f"this build of the library has no {name}")
    with torch.cuda.device(src.device):
        rc = getattr(lib, name)(action._perm_c, action._sign_c, action.n_elements, action.n_units, action.width, src.data_ptr(), int(windows), dst.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream))
    eng._check(lib, rc, name)


class _OrbitAverageFn(torch.autograd.Function):
    """mshgnn_orbit_average / mshgnn_orbit_average_backward on the current stream; the gradient reaches the engine through whatever produced `out`."""

    @staticmethod
    def forward(ctx, out, action, windows):
        o = _as_rows(out, action, windows)
        avg = torch.empty(windows, action.row, dtype=torch.float32, device=o.device)
        _launch("mshgnn_orbit_average", action, o, windows, avg)
        ctx.action, ctx.windows, ctx.like = action, windows, (out.shape, out.dtype)
        return avg

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        action, windows = ctx.action, ctx.windows
        g32 = g.contiguous().to(torch.float32)
        go = torch.empty(action.n_elements * windows, action.row, dtype=torch.float32, device=g32.device)
        _launch("mshgnn_orbit_average_backward", action, g32, windows, go)
        shape, dtype = ctx.like
        return go.to(dtype).view(shape), None, None


def orbit_average(out: torch.Tensor, action: OutputAction, windows: int) -> torch.Tensor:
    """avg [windows, n_units . width] (fp32) of the outputs `out` of an orbit-complete batch (K . windows . n_units . width values in element-major window order;
    any shape, made contiguous fp32 as the engine's entry points do): avg[w] = 1/K . sum_e rho_out(g_e)^-1 out[e . windows + w], the adds in element order and one
    multiply by fl32(1/K) (include/mshgnn.h).  Differentiable once; works under torch.no_grad()."""
    return _OrbitAverageFn.apply(out, action, int(windows))


class EquivarianceDefect:
    """The equivariance defect ||rho_out(g)^-1 f(g x) - f(x)|| of a model, per operator, accumulated over a sweep of orbit-complete batches: one launch per
    `update` into an fp64 device state [K][4] = {sum d^2, sum f(x)^2, max |d|, count}; `report` synchronises once."""

    def __init__(self, action: OutputAction, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("the equivariance defect runs on a HIP device; there is no CPU fallback")
        self.action = action
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros(action.n_elements, 4, dtype=torch.float64, device=self.device)

    @property
    def operators(self) -> List[str]:
        """the names of the elements 1 .. K - 1, in element order"""
        return [str(op) for op in self.action.operators[1:]]

    def reset(self) -> None:
        self.state.zero_()

    def update(self, out: torch.Tensor, windows: int) -> None:
        _launch("mshgnn_orbit_defect", self.action, _as_rows(out, self.action, windows), windows, self.state)

    def report(self) -> Dict[str, Dict[str, float]]:
        """{operator: {"rms": sqrt(sum d^2 / n), "max_abs": max |d|, "relative_rms": sqrt(sum d^2 / sum f(x)^2), "n": values compared}} -- one host read."""
        st = self.state.cpu().tolist()
        res = {}
        for name, (sd, s0, mx, n) in zip(self.operators, st[1:]):
            res[name] = {"rms": math.sqrt(sd / n) if n else 0.0, "max_abs": mx, "relative_rms": math.sqrt(sd / s0) if s0 else (0.0 if sd == 0 else math.inf),
                         "n": int(n)}
        return res


# ---- a wrapper whose steps run on the symmetrised prediction ---------------------------------------------------------------------------------------------

def _raw_step(wrapper, batch):
    """(y, y_pred) of the RAW model on `batch`, for a wrapper or its `Symmetrised` view."""
    cls = getattr(wrapper, "_raw_class", type(wrapper))
    return cls.step_helper_function(wrapper, batch)


class _SymmetrisedSteps:
    """Mixed in FRONT of a wrapper's class by `Symmetrised`: the one method every step goes through."""

    fused_training_step = False      # the one-call engine steps compute the raw model's loss, not the symmetrised one: always the two-call route

    def step_helper_function(self, batch):
        action = self.output_action
        K, row = action.n_elements, action.row
        n = int(batch.batch_size) if hasattr(batch, "batch_size") else int(batch[0].shape[0])
        if n % K:
            raise ValueError(f"a symmetrised step takes an orbit-complete batch: {n} windows are no multiple of the {K} group elements")
        B = n // K
        y, y_pred = _raw_step(self, batch)      # forward_windows under no_grad, the ordinary autograd forward otherwise
        if y_pred.numel() != n * row:
            raise ValueError(f"the model's output has {y_pred.numel() // max(n, 1)} values per window, the output action {row}")
        avg = orbit_average(y_pred.reshape(n, row), action, B)
        return y[:B], avg.view(B, *y_pred.shape[1:])


def Symmetrised(wrapper, action: OutputAction):
    """A view of `wrapper` (the GRF wrappers `Heterogeneous_GNN_Lightning`, `HGNN_K4_Lightning`, `HGNN_C2_Lightning_Reg`, `HGNN_C2_Lightning_Cls`, and
    `MLP_Lightning`) whose `step_helper_function` runs the wrapped model on an ORBIT-COMPLETE batch and returns the labels of its first B windows with the
    orbit-averaged prediction: `training_step` / `validation_step` / `test_step` / `predict_step`, the metric state and the flat optimizers work on it unchanged,
    the backward reaches the engine through the two-call route.  The view shares the model (its parameters) with `wrapper` and keeps metric state and `logged`
    of its own; `view.raw` is `wrapper`.  `fused_training_step` is off: that step's loss is the raw model's.  The training loss is the shared model's
    (`set_regression_loss` on the wrapper, the view or the model: one setting, kept on the model, which every wrapper over it reads per step): L1 / Huber on the
    AVERAGED prediction, through the stand-alone loss operator.  `grf_body_to_world_frame` is refused (the
    world-frame metrics would pair K . B quaternions with B predictions).

    The centroidal-momentum wrappers (`COM_HGNN_SYM_Lightning`, `COM_HGNN_Lightning`, `COM_MLP_Lightning`) are taken with the action of a Solo orbit made from
    `symmetry=True` recipes: width 1 and a row of `num_bases * 6` units; the labels of the first B windows and the averaged prediction go through
    `ComStepMetrics` as any batch does.  Of these models only `COM_HGNN_K4` (gs, gt, gr) and `COM_HGNN_C2` (gs) are equivariant ARCHITECTURES, and only on the
    dataset's zero base series (the COM models mask the joints only): their symmetrised view changes nothing but rounding.  `COM_HGNN_S4`, `COM_HGNN` and the
    MLP are the baselines one symmetrises."""
    from . import wrappers
    if isinstance(wrapper, wrappers.COM_Base_Lightning):
        if not isinstance(action, OutputAction):
            raise TypeError("action must be an OutputAction")
        row = int(wrapper.model.num_bases) * 6
        if action.width != 1 or action.row != row:
            raise ValueError(f"this centroidal-momentum (COM) wrapper has {row} outputs per window (num_bases * 6): it needs an output action of width 1 over "
                             f"{row} units (a Solo orbit of symmetry=True recipes), not {action.n_units} units of width {action.width}")
    elif not isinstance(wrapper, (wrappers._HGNNWrapper, wrappers.MLP_Lightning)):
        raise TypeError(f"Symmetrised takes a GRF wrapper, a COM wrapper or MLP_Lightning, not {type(wrapper).__name__}")
    if getattr(wrapper, "body_to_world_frame", False):
        raise ValueError("Symmetrised does not take grf_body_to_world_frame=True: evaluate the symmetrised predictions in the body frame")
    if not isinstance(action, OutputAction):
        raise TypeError("action must be an OutputAction")
    raw_cls = getattr(wrapper, "_raw_class", type(wrapper))
    width = 2 if not wrapper.regression else 1
    if action.width != width:
        raise ValueError(f"the output action has width {action.width}; a {'regression' if wrapper.regression else 'classification'} wrapper needs {width}")
    view = copy.copy(wrapper)      # shares _parameters / _modules (the model) by reference
    view.__class__ = type("Symmetrised" + raw_cls.__name__, (_SymmetrisedSteps, raw_cls), {"_raw_class": raw_cls})
    view.__dict__["fused_training_step"] = False      # on the INSTANCE: a per-wrapper `w.fused_training_step = True` was copied with the rest and would shadow the class's
    view.__dict__["_metrics"] = None
    view.__dict__["_metrics_world"] = None
    view.__dict__["logged"] = {}
    view.__dict__["output_action"] = action
    view.__dict__["raw"] = wrapper
    return view


def evaluate_sequence_symmetrised(wrapper, orbit_store_or_view, edge_index_dict, batch_size: int, stride: int = 1, action: Optional[OutputAction] = None):
    """One sweep under torch.no_grad() over the base windows 0, stride, 2 stride, ... of an `orbit` store (or of a `DatasetView` / `ResidentDataset` of an orbit
    dataset: its base-window indices), `batch_size` BASE windows per batch (K times as many model rows, the last batch ragged): returns
    (the symmetrised predictions [n, ...] in window order, the `EquivarianceDefect.report()` of the RAW model over the same sweep).  wrapper: a raw wrapper or
    its `Symmetrised` view (whose action is used); action: default `OutputAction.from_store`.  edge_index_dict: one window's edges or a callable, as
    `wrappers.evaluate_sequence` takes them."""
    from . import wrappers
    from .windows import DatasetView, ResidentDataset
    if batch_size < 1 or stride < 1:
        raise ValueError("batch_size and stride must be >= 1")
    src = orbit_store_or_view.view() if isinstance(orbit_store_or_view, ResidentDataset) else orbit_store_or_view
    store = src.dataset if isinstance(src, DatasetView) else src
    if action is None:
        action = getattr(wrapper, "output_action", None) or OutputAction.from_store(store, bool(wrapper.regression))
    K, row = action.n_elements, action.row
    if int(store.n_elements) != K:
        raise ValueError(f"the store's orbit has {store.n_elements} elements, the output action {K}")
    n = src.n_windows if isinstance(src, DatasetView) else len(src)
    base = torch.arange(0, n, stride, dtype=torch.int64, device=store.device)
    edges_for = wrappers.tiled_edges(store, edge_index_dict)
    defect = EquivarianceDefect(action, store.device)
    preds = []
    with torch.no_grad():
        for lo in range(0, int(base.numel()), batch_size):
            ix = base[lo:lo + batch_size]
            B = int(ix.numel())
            batch = src.orbit_batch(ix, edges_for(K * B))
            _, y_pred = _raw_step(wrapper, batch)
            o = y_pred.reshape(K * B, row)
            defect.update(o, B)
            preds.append(orbit_average(o, action, B).view(B, *y_pred.shape[1:]))
    if isinstance(src, DatasetView):
        src.check()
    return torch.cat(preds, 0), defect.report()
