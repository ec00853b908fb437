"""On-device window assembly: a sequence's raw time series live on the GPU and a minibatch of time windows is gathered
straight into the engine's input layout by `mshgnn_assemble_windows` (include/mshgnn.h).

This is the device counterpart of the reference's per-window Python path (relative to /root/reference/src/ms_hgnn):
datasets_py/quadSDKDataset_Morph.py:99-175 (`load_data_sorted_c2`), :304-369 (`get_helper_heterogeneous_gnn_c2`),
:444-489 (`load_data_at_dataset_seq[_3d]`), datasets_py/flexibleDataset.py:340-400, 563-596 and PyG's collate -- i.e.
`DataLoader(dataset, batch_size=B)` -> `batch.x_dict`, `batch.y`, `batch.r_o` for B window indices at once.

A `WindowRecipe` says, per node type, which columns of which raw series become the T-long runs of a node's feature row
(variable-major, axis-major: the reference's `flatten('F')` layout); types without variables are all-ones of width 1
(flexibleDataset.py:183-190).  No CPU implementation: without a HIP device `SequenceStore` raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import os

import numpy as np
import torch

from . import engine as eng


@dataclass
class WindowRecipe:
    node_types: List[str]
    num_nodes: Dict[str, int]
    history: int                                            # T
    # per type: list of variables; a variable = (series name, columns[node][axis])
    variables: Dict[str, List[Tuple[str, List[List[int]]]]]
    label_series: Optional[str] = None
    label_cols: List[int] = field(default_factory=list)
    label_rotate: bool = False                              # 3-D world-frame labels -> body frame (needs quat_series)
    quat_series: Optional[str] = None
    normalize: bool = False                                 # per-window standardisation (flexibleDataset.py:390-396)
    # group-transformed windows (`transformed`): which part of the morphological symmetry group acts on a series' columns, and the +-1 a run / a label carries
    symmetry_parts: Optional[Dict[str, str]] = None         # series name -> "js" | "fs" | "bs_lin" | "bs_ang" | "ls" (labels also: the compound "bs_linang")
    variable_signs: Optional[Dict[str, List[List[List[int]]]]] = None      # per type: [variable][node][axis] of +-1, mirroring `variables` (None: all +1)
    label_signs: Optional[List[int]] = None                 # [n_label] of +-1 (None: all +1)
    # the position of every label in the UNTRANSFORMED recipe, permuted with the labels by `transformed` (host-only: not in `tables()` or the descriptor).
    # It names a label where its column cannot: the Solo labels repeat the 6 columns of Y once per base node (`symmetrise.OutputAction.from_recipes`)
    label_slots: Optional[List[int]] = None

    def _linang_table(self, operator: str, group: "GroupAction", mode: str) -> Tuple[List[int], List[int]]:
        """(P, c) of the compound label part "bs_linang" over this recipe's labels [n_base][lin(3) | ang(3)]: slot 6 node + a takes entry 3 node + a of the
        'bs_lin' table for a < 3 and entry 3 node + (a - 3) of 'bs_ang' otherwise -- the base nodes permuted by `permutation_Q_bs`, the lin halves reflected by
        `reflection_Q_bs_lin`, the ang halves by `reflection_Q_bs_ang`.  ONE copy (6 labels) against tables tiled over 2 or 4 base nodes: the copy's own
        reflection, no permutation (the `one_node` rule of the variables)."""
        n = len(self.label_cols)
        (P, cl), (_, ca) = group.table("bs_lin", operator, mode), group.table("bs_ang", operator, mode)
        if n % 6 or len(P) % 3:
            raise ValueError(f"labels '{self.label_series}': the 'bs_linang' part acts on [n_base][lin(3) | ang(3)] labels, not on {n}")
        nb, nt = n // 6, len(P) // 3
        if any(P[3 * j + i] != P[3 * j] + i or P[3 * j] % 3 for j in range(nt) for i in range(3)):
            raise ValueError("bs_linang: the base permutation must map node triples to node triples in axis order")
        if nb == 1 and nt != 1 and all(c[k] == c[k % 3] for c in (cl, ca) for k in range(len(P))):
            nodes = [0]
        elif nb == nt:
            nodes = [P[3 * j] // 3 for j in range(nb)]
        else:
            raise ValueError(f"labels '{self.label_series}': {nb} base nodes, but the group's 'bs' tables have {nt}")
        return ([6 * nodes[k // 6] + k % 6 for k in range(n)],
                [int(cl[3 * (k // 6) + k % 6] if k % 6 < 3 else ca[3 * (k // 6) + k % 6 - 3]) for k in range(n)])

    def transformed(self, operator: str, group: "GroupAction", mode: str = "MorphSym") -> "WindowRecipe":
        """The recipe of g . window for g = operator in ("gs", "gt", "gr"): what the reference's dataset classes build with `symmetry_operator`
        (quadSDKDataset_Morph.py:113-159, 177-239; LinTzuYaunDataset_Morph.py:294-333, 349-408) -- every sorted part X [T, n] becomes
        X'[:, k] = c[k] X[:, P[k]] over its flat index k = node * n_axes + axis, BEFORE standardisation; labels likewise, AFTER the body-frame
        rotation; the quaternion by-product is left alone.  The permutation is a choice of columns, the reflection a sign per run / label
        (`variable_signs`, `label_signs`), so the transformed windows come out of the same resident series.  Composes: the result can be
        transformed again."""
        perm_of = {}
        def table(part, n, what, one_node=False):
            if part not in perm_of:
                perm_of[part] = group.table(part, operator, mode)
            P, c = perm_of[part]
            if one_node and len(P) != n and n > 0 and len(P) % n == 0 and all(P[k] % n == k % n and c[k] == c[k % n] for k in range(len(P))):
                # the part's tables are tiled over copies of ONE n-vector (the base series, tiled to the graph models' base nodes) and this variable is a
                # single node holding one copy (`mlp_recipe`: lin_acc / ang_vel are [T, 3]): the action on one copy -- no permutation, the copy's reflection
                P, c = list(range(n)), list(c[:n])
            if len(P) != n:
                raise ValueError(f"{what}: {n} columns, but the group's '{part}' tables have {len(P)}")
            return P, c
        if operator not in GroupAction.OPERATORS:
            raise ValueError(f"unknown symmetry operator {operator!r}: one of {GroupAction.OPERATORS}")
        if mode not in GroupAction.MODES:
            raise ValueError(f"unknown symmetry mode {mode!r}: one of {GroupAction.MODES}")
        if self.symmetry_parts is None:
            raise ValueError("this recipe does not say which part of the group acts on its series (symmetry_parts is None); the Solo-12 recipes name theirs only "
                             "when made with symmetry=True: the reference's own loader cannot run there, it hands apply_symmetry a Python list "
                             "(soloDataset.py:619-623, 722-739)")
        variables, signs = {}, {}
        for t in self.node_types:
            variables[t], signs[t] = [], []
            old_signs = (self.variable_signs or {}).get(t)
            for vi, (s, cols) in enumerate(self.variables.get(t, [])):
                if s not in self.symmetry_parts:
                    raise ValueError(f"series '{s}' has no entry in symmetry_parts")
                na = len(cols[0])
                flat = [c for node in cols for c in node]
                fsig = [x for node in old_signs[vi] for x in node] if old_signs else [1] * len(flat)
                P, c = table(self.symmetry_parts[s], len(flat), f"variable '{s}' of type '{t}'", one_node=len(cols) == 1)
                nflat = [flat[P[k]] for k in range(len(flat))]
                nsig = [int(c[k]) * int(fsig[P[k]]) for k in range(len(flat))]
                variables[t].append((s, [nflat[i:i + na] for i in range(0, len(nflat), na)]))
                signs[t].append([nsig[i:i + na] for i in range(0, len(nsig), na)])
        label_cols, label_signs, label_slots = list(self.label_cols), self.label_signs, self.label_slots
        if self.label_cols:
            if self.label_series not in self.symmetry_parts:
                raise ValueError(f"label series '{self.label_series}' has no entry in symmetry_parts")
            if self.symmetry_parts[self.label_series] == "bs_linang":
                P, c = self._linang_table(operator, group, mode)
            else:
                P, c = table(self.symmetry_parts[self.label_series], len(self.label_cols), f"labels '{self.label_series}'")
            if self.label_rotate and any(P[3 * j + i] != P[3 * j] + i or P[3 * j] % 3 for j in range(len(P) // 3) for i in range(3)):
                # the rotation acts on whole (x, y, z) triples of one foot BEFORE the transform: the permuted columns must still be such triples
                raise ValueError("label_rotate: the label permutation must map foot triples to foot triples in axis order")
            old = self.label_signs or [1] * len(self.label_cols)
            label_cols = [self.label_cols[P[k]] for k in range(len(P))]
            label_signs = [int(c[k]) * int(old[P[k]]) for k in range(len(P))]
            if self.label_slots is not None:
                label_slots = [self.label_slots[P[k]] for k in range(len(P))]
        return dataclasses.replace(self, variables=variables, variable_signs=signs, label_cols=label_cols, label_signs=label_signs, label_slots=label_slots)

    def width(self, t: str) -> int:
        w = sum(len(cols[0]) * self.history for _, cols in self.variables.get(t, []))
        return w if w > 0 else 1

    def tables(self, names: Optional[Sequence[str]] = None, n_columns: Optional[Dict[str, int]] = None) -> Tuple[List[List[int]], List[List[int]], List[int], bool]:
        """The tables of include/mshgnn.h's mshgnn_window_desc for this recipe, on the host: (runs [n_runs][5], rows [n_rows][2], label_cols, signed).
        names: the order of the source arrays (None: `series()`); n_columns: series name -> its number of columns, checked when given (a store knows them).
        A negated run / label carries SIGN_FLAG in its source word / column; `signed` says whether any does."""
        names = list(names) if names is not None else self.series()
        sidx = {s: i for i, s in enumerate(names)}
        def ncol_of(s):
            return min(int(n_columns[s]), 256) if n_columns is not None else 256
        runs, rows = [], []
        signed = False
        for ti, t in enumerate(self.node_types):
            vars_ = self.variables.get(t, [])
            if not vars_:
                for n in range(self.num_nodes[t]):
                    rows.append([len(runs), len(runs) + 1]); runs.append([ti, n, 0, -1, 1])
                continue
            vsig = (self.variable_signs or {}).get(t)
            for n in range(self.num_nodes[t]):
                f = 0
                r_begin = len(runs)
                for vi, (s, cols) in enumerate(vars_):
                    for ai, c in enumerate(cols[n]):
                        if not 0 <= c < ncol_of(s):
                            raise ValueError(f"column {c} of series '{s}' out of range")
                        sg = int(vsig[vi][n][ai]) if vsig else 1
                        if sg not in (-1, 1):
                            raise ValueError(f"variable_signs of series '{s}': {sg} is not +-1")
                        signed |= sg < 0
                        runs.append([ti, n, f, (sidx[s] << 8) | c | (SIGN_FLAG if sg < 0 else 0), self.history])
                        f += self.history
                rows.append([r_begin, len(runs)])
        lab = list(self.label_cols or [0])
        if self.label_cols:
            for c in lab:
                if not 0 <= c < ncol_of(self.label_series):
                    raise ValueError(f"label column {c} of series '{self.label_series}' out of range")
        if self.label_signs is not None and self.label_cols:
            if len(self.label_signs) != len(self.label_cols) or any(int(x) not in (-1, 1) for x in self.label_signs):
                raise ValueError("label_signs: one +-1 per label column")
            signed |= any(int(x) < 0 for x in self.label_signs)
            lab = [c | (SIGN_FLAG if int(x) < 0 else 0) for c, x in zip(lab, self.label_signs)]
        return runs, rows, lab, signed

    def orbit(self, group: "GroupAction", operators: Sequence[str] = ("gs", "gt", "gr"), mode: str = "MorphSym", identity: bool = True) -> List["WindowRecipe"]:
        """The recipes of an orbit batch's group elements, in element order: this recipe (identity=True), then `transformed(op)` for every operator --
        the datasets of the reference's ConcatDataset([ds, ds_gs, ds_gt, ds_gr]).  1 to MAX_ELEMENTS elements."""
        recipes = ([self] if identity else []) + [self.transformed(op, group, mode) for op in operators]
        if not 1 <= len(recipes) <= MAX_ELEMENTS:
            raise ValueError(f"an orbit has 1 to {MAX_ELEMENTS} group elements, not {len(recipes)}")
        return recipes

    def series(self) -> List[str]:
        names = []
        for t in self.node_types:
            for s, _ in self.variables.get(t, []):
                if s not in names:
                    names.append(s)
        for s in (self.label_series, self.quat_series):
            if s is not None and s not in names:
                names.append(s)
        return names


SIGN_FLAG = 1 << 30          # MSHGNN_WINDOW_SIGN_FLAG: a run's source word / a label column carries a minus sign
MAX_ELEMENTS = 8             # MSHGNN_WINDOW_MAX_ELEMENTS: group elements of an orbit descriptor
ELEMENT_SHIFT = 56           # MSHGNN_START_ELEMENT_SHIFT: a packed start = element << 56 | row
ROW_MASK = (1 << ELEMENT_SHIFT) - 1


def stack_orbit_tables(tables: Sequence[Tuple[List[List[int]], List[List[int]], List[int]]]) -> Tuple[List[List[List[int]]], List[List[int]], List[List[int]]]:
    """The element-major tables of an orbit descriptor from the (runs, rows, label_cols) of its K elements (`WindowRecipe.tables`): (runs [K][n_runs][5],
    rows, label_cols [K][n_label]).  All elements share their row structure, which is what lets a window pick its element inside the gathers; refused
    here as the library's checking call refuses it: more than MAX_ELEMENTS elements, an element whose rows or whose {type, node, first feature, length}
    of any run differ from element 0's, a constant-1 run (source word -1) that is not constant-1 in every element."""
    K = len(tables)
    if not 1 <= K <= MAX_ELEMENTS:
        raise ValueError(f"an orbit has 1 to {MAX_ELEMENTS} group elements, not {K}")
    runs0, rows0, lab0 = tables[0]
    for e, (runs, rows, lab) in enumerate(tables):
        if [list(r) for r in rows] != [list(r) for r in rows0] or len(runs) != len(runs0):
            raise ValueError(f"orbit element {e}: its node rows differ from element 0's")
        if len(lab) != len(lab0):
            raise ValueError(f"orbit element {e}: {len(lab)} label columns, element 0 has {len(lab0)}")
        for r, (a, b) in enumerate(zip(runs, runs0)):
            if [a[0], a[1], a[2], a[4]] != [b[0], b[1], b[2], b[4]]:
                raise ValueError(f"orbit element {e}, run {r}: (type, node, first feature, length) = {[a[0], a[1], a[2], a[4]]} differs from element 0's {[b[0], b[1], b[2], b[4]]}")
            if (a[3] == -1) != (b[3] == -1) or (a[3] < 0 and a[3] != -1):
                raise ValueError(f"orbit element {e}, run {r}: a constant-1 run must be the constant-1 run (source word -1) in every element")
    return [[list(r) for r in t[0]] for t in tables], [list(r) for r in rows0], [list(t[2]) for t in tables]


def orbit_index_split(index: int, n_windows: int, n_elements: int) -> Tuple[int, int]:
    """(element, window) of index `index` of an orbit view over n_windows windows: element index // n, window index % n -- the order of
    ConcatDataset([view, view_gs, view_gt, view_gr]).  IndexError outside [0, n_elements * n_windows)."""
    i = int(index)
    if not 0 <= i < n_elements * n_windows:
        raise IndexError(f"dataset index {i} out of range [0, {n_elements * n_windows})")
    return i // n_windows, i % n_windows


@dataclass
class GroupAction:
    """The tables of a morphological symmetry group file (morphsym_hgnn_amd/cfg/*.yaml): per part an index permutation (`permutation_Q_*`) and a +-1
    reflection (`reflection_Q_*`), row 0 = sagittal (gs), row 1 = transversal (gt).  The base has one permutation and two reflections (linear /
    angular series)."""
    permutation: Dict[str, List[List[int]]]      # "js" | "fs" | "bs" | "ls" -> [2][n]
    reflection: Dict[str, List[List[int]]]       # "js" | "fs" | "bs_lin" | "bs_ang" | "ls" -> [2][n]
    name: str = ""

    OPERATORS = ("gs", "gt", "gr")
    MODES = ("MorphSym", "Euclidean")
    PARTS = {"js": "js", "fs": "fs", "bs_lin": "bs", "bs_ang": "bs", "ls": "ls"}      # reflection key -> permutation key

    @classmethod
    def load(cls, name_or_path: str) -> "GroupAction":
        """A path, or the stem of a file in the package's cfg/ ("a1-c2", "mini_cheetah-k4")."""
        import yaml
        path = name_or_path
        if not os.path.isfile(path):
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cfg", f"{name_or_path}.yaml")
        if not os.path.isfile(path):
            raise ValueError(f"no group file '{name_or_path}' (a path, or the stem of a file in cfg/)")
        with open(path) as f:
            d = yaml.safe_load(f)
        # (a robot without some part -- the Solo files have no foot tables -- simply lacks those keys: `table` says so when asked for them)
        perm = {k: [[int(x) for x in row] for row in d[f"permutation_Q_{k}"]] for k in ("js", "fs", "bs", "ls") if f"permutation_Q_{k}" in d}
        refl = {k: [[int(x) for x in row] for row in d[f"reflection_Q_{k}"]] for k, pk in cls.PARTS.items() if f"reflection_Q_{k}" in d and pk in perm}
        for k in refl:
            pk = cls.PARTS[k]
            for row_p, row_c in zip(perm[pk], refl[k]):
                if sorted(row_p) != list(range(len(row_p))) or len(row_c) != len(row_p) or any(x not in (-1, 1) for x in row_c):
                    raise ValueError(f"group file '{name_or_path}': '{k}' is no permutation with +-1 reflections")
        return cls(perm, refl, os.path.splitext(os.path.basename(path))[0])

    def table(self, part: str, operator: str, mode: str = "MorphSym") -> Tuple[List[int], List[int]]:
        """(P, c) with X'[k] = c[k] X[P[k]]: gs -> (P0, c_gs), gt -> (P1, c_gt), gr -> (P0[P1[k]], c_gs c_gt); mode "Euclidean": c is all ones
        (the reference's create_coefficient_dict)."""
        if part not in self.PARTS:
            raise ValueError(f"unknown group part {part!r}: one of {tuple(self.PARTS)}")
        if operator not in self.OPERATORS:
            raise ValueError(f"unknown symmetry operator {operator!r}: one of {self.OPERATORS}")
        if mode not in self.MODES:
            raise ValueError(f"unknown symmetry mode {mode!r}: one of {self.MODES}")
        if part not in self.reflection:
            raise ValueError(f"group '{self.name}' has no '{part}' tables")
        (P0, P1), (c0, c1) = self.permutation[self.PARTS[part]], self.reflection[part]
        if operator == "gs":
            P, c = list(P0), list(c0)
        elif operator == "gt":
            P, c = list(P1), list(c1)
        else:
            P, c = [P0[P1[k]] for k in range(len(P0))], [c0[k] * c1[k] for k in range(len(c0))]
        return P, (c if mode == "MorphSym" else [1] * len(c))


def quadsdk_a1_c2_recipe(joint_perm: Sequence[int], foot_perm: Sequence[int], history: int = 150, grf_dimension: int = 3,
                         body_frame_labels: bool = False, normalize: bool = False, n_base: int = 2) -> WindowRecipe:
    """The A1 / Quad-SDK C2 dataset (BASELINE config): base = tiled IMU (lin acc, ang vel), joint = (q, qd, tau) in graph
    order, feet = ones; labels = GRFs of the window's last step in foot order (quadSDKDataset_Morph.py:99-160, 304-369)."""
    if grf_dimension == 3:
        lab = [int(3 * i + k) for i in foot_perm for k in range(3)]
    elif grf_dimension == 1:
        lab = [int(3 * i + 2) for i in foot_perm]
    else:
        raise ValueError("grf_dimension must be 1 or 3")
    if body_frame_labels and grf_dimension != 3:
        # the reference rotates the 3-D GRFs first and then keeps z; on device that is the rotated z, which needs all three
        raise ValueError("body-frame labels need grf_dimension == 3")
    return WindowRecipe(
        node_types=["base", "joint", "foot"], num_nodes={"base": n_base, "joint": len(joint_perm), "foot": len(foot_perm)},
        history=history,
        variables={"base": [("imu_acc", [[0, 1, 2]] * n_base), ("imu_omega", [[0, 1, 2]] * n_base)],
                   "joint": [(s, [[int(j)] for j in joint_perm]) for s in ("q", "qd", "tau")], "foot": []},
        label_series="F", label_cols=lab, label_rotate=body_frame_labels, quat_series="r_o", normalize=normalize,
        # (3-D GRFs transform like foot vectors, 1-D ones like labels: apply_symmetry(part='label'), quadSDKDataset_Morph.py:204-211)
        symmetry_parts={"imu_acc": "bs_lin", "imu_omega": "bs_ang", "q": "js", "qd": "js", "tau": "js", "F": "fs" if grf_dimension == 3 else "ls"})


def minicheetah_k4_recipe(joint_perm: Sequence[int], foot_perm: Sequence[int], history: int = 150, normalize: bool = False,
                          n_base: int = 4) -> WindowRecipe:
    """The MiniCheetah (LinTzuYaun) contact dataset on the K4 graph: base = IMU tiled to the 4 base nodes, joint = (q, qd) in
    graph order, foot = (p, v) 3-D in foot order; labels = contact flags of the window's last step in foot order
    (LinTzuYaunDataset.py:65-88, LinTzuYaunDataset_Morph.py:251-347, 555-625)."""
    fcols = [[int(3 * i + k) for k in range(3)] for i in foot_perm]
    return WindowRecipe(
        node_types=["base", "joint", "foot"], num_nodes={"base": n_base, "joint": len(joint_perm), "foot": len(foot_perm)}, history=history,
        variables={"base": [("imu_acc", [[0, 1, 2]] * n_base), ("imu_omega", [[0, 1, 2]] * n_base)],
                   "joint": [(s, [[int(j)] for j in joint_perm]) for s in ("q", "qd")],
                   "foot": [("p", fcols), ("v", fcols)]},
        label_series="contacts", label_cols=[int(i) for i in foot_perm], normalize=normalize,
        symmetry_parts={"imu_acc": "bs_lin", "imu_omega": "bs_ang", "q": "js", "qd": "js", "p": "fs", "v": "fs", "contacts": "ls"})


# What the group acts on in the Solo recipes made with symmetry=True (cfg/solo-k4.yaml, cfg/solo-c2.yaml): q / qd by the `js` tables, the base series by `bs`
# with its lin / ang reflections, the labels [n_base][lin(3) | ang(3)] by the compound part "bs_linang" (`WindowRecipe._linang_table`).
SOLO_SYMMETRY_PARTS = {"q": "js", "qd": "js", "base_lin": "bs_lin", "base_ang": "bs_ang", "Y": "bs_linang"}


def solo_com_recipe(kind: str, joint_perm: Sequence[int], history: int = 1, symmetry: bool = False) -> WindowRecipe:
    """The Solo-12 centroidal-momentum dataset (BASELINE configs[3] data format) on the K4 / C2 / S4 graphs: joint = (q, qd) in graph
    order, base = the (all-zero) IMU series tiled to the base nodes, labels = the 6-D base velocity of the window's last row, once per
    base node as [lin(3) | ang(3)] (soloDataset.py:235-300, 382-400, 546-717).  Series: `solo_com_arrays(X, Y)`.
    symmetry=True: the recipe names the group parts of its series (`SOLO_SYMMETRY_PARTS`) and tracks its label slots, so `transformed` / `orbit` and
    `symmetrise.OutputAction.from_recipes` take it; the default recipe stays the reference's (its own loader cannot transform these windows)."""
    nb = {"k4_com": 4, "c2_com": 2, "s4_com": 1}[kind]
    return WindowRecipe(
        node_types=["base", "joint"], num_nodes={"base": nb, "joint": len(joint_perm)}, history=history,
        variables={"base": [("base_lin", [[0, 1, 2]] * nb), ("base_ang", [[0, 1, 2]] * nb)],
                   "joint": [(s, [[int(j)] for j in joint_perm]) for s in ("q", "qd")]},
        label_series="Y", label_cols=[0, 1, 2, 3, 4, 5] * nb,
        symmetry_parts=dict(SOLO_SYMMETRY_PARTS) if symmetry else None, label_slots=list(range(6 * nb)) if symmetry else None)


MLP_NODE_TYPE = "mlp"


def mlp_recipe(variables: Sequence[Tuple[str, Sequence[int]]], history: int, label_series: Optional[str] = None, label_cols: Sequence[int] = (),
               label_rotate: bool = False, quat_series: Optional[str] = None, normalize: bool = False,
               symmetry_parts: Optional[Dict[str, str]] = None) -> WindowRecipe:
    """The input of the reference's MLP baseline (flexibleDataset.get_helper_mlp, flexibleDataset.py:510-535): the concatenation, variable by variable, of
    X.flatten('F') of the sorted [T, n] arrays -- every column's T steps contiguous.  That is ONE node type holding ONE node whose variables list all
    columns: each (variable, column) becomes one run of `history` elements at consecutive feature offsets, so every window route serves it unchanged.
    variables: (series name, columns) in the reference's order [lin_acc, ang_vel, j_p, j_v, j_T, f_p, f_v]; absent (None / empty) variables are skipped."""
    vars_ = [(s, [[int(c) for c in cols]]) for s, cols in variables if s is not None and cols is not None and len(cols) > 0]
    if not vars_:
        raise ValueError("an MLP recipe needs at least one variable")
    return WindowRecipe(node_types=[MLP_NODE_TYPE], num_nodes={MLP_NODE_TYPE: 1}, history=history, variables={MLP_NODE_TYPE: vars_},
                        label_series=label_series, label_cols=[int(c) for c in label_cols], label_rotate=label_rotate, quat_series=quat_series,
                        normalize=normalize, symmetry_parts=symmetry_parts)


def quadsdk_a1_mlp_recipe(joint_perm: Sequence[int], foot_perm: Sequence[int], history: int = 150, grf_dimension: int = 3,
                          body_frame_labels: bool = False, normalize: bool = False) -> WindowRecipe:
    """The A1 / Quad-SDK dataset as the MLP baseline reads it: in = history x 42 (lin acc 3, ang vel 3, q / qd / tau 12 each in sorted joint order); series
    names, labels and symmetry parts of `quadsdk_a1_c2_recipe`."""
    g = quadsdk_a1_c2_recipe(joint_perm, foot_perm, history, grf_dimension, body_frame_labels, normalize)
    jp = [int(j) for j in joint_perm]
    return mlp_recipe([("imu_acc", [0, 1, 2]), ("imu_omega", [0, 1, 2]), ("q", jp), ("qd", jp), ("tau", jp)], history, g.label_series, g.label_cols,
                      g.label_rotate, g.quat_series, normalize, g.symmetry_parts)


def minicheetah_mlp_recipe(joint_perm: Sequence[int], foot_perm: Sequence[int], history: int = 150, normalize: bool = False) -> WindowRecipe:
    """The MiniCheetah contact dataset as the MLP baseline reads it: in = history x 54 (lin acc, ang vel, q, qd, foot p, foot v); series names, labels and
    symmetry parts of `minicheetah_k4_recipe`."""
    g = minicheetah_k4_recipe(joint_perm, foot_perm, history, normalize)
    jp = [int(j) for j in joint_perm]
    fc = [int(3 * i + k) for i in foot_perm for k in range(3)]
    return mlp_recipe([("imu_acc", [0, 1, 2]), ("imu_omega", [0, 1, 2]), ("q", jp), ("qd", jp), ("p", fc), ("v", fc)], history, g.label_series, g.label_cols,
                      False, None, normalize, g.symmetry_parts)


def solo_com_mlp_recipe(joint_perm: Sequence[int], history: int = 1, symmetry: bool = False) -> WindowRecipe:
    """The Solo-12 centroidal-momentum dataset as the MLP baseline reads it (gnnLightning_com.py:234-287): in = history x 24 (q | qd), labels = the 6-D base
    velocity of the window's last row; series names of `solo_com_recipe` / `solo_com_arrays`; symmetry: as there (6 labels: one copy's reflection)."""
    jp = [int(j) for j in joint_perm]
    r = mlp_recipe([("q", jp), ("qd", jp)], history, "Y", [0, 1, 2, 3, 4, 5], symmetry_parts=dict(SOLO_SYMMETRY_PARTS) if symmetry else None)
    return dataclasses.replace(r, label_slots=list(range(6))) if symmetry else r


def solo_com_arrays(X: np.ndarray, Y: np.ndarray) -> Dict[str, np.ndarray]:
    """The raw series `solo_com_recipe` names, from the dataset's X [N, 24] (q | qd) and Y [N, 6] (soloDataset.py:382-400: the base
    IMU inputs of this task are zeros)."""
    X, Y = np.asarray(X), np.asarray(Y)
    z = np.zeros((X.shape[0], 3), dtype=np.float32)
    return {"q": X[:, :12], "qd": X[:, 12:], "base_lin": z, "base_ang": z, "Y": Y}


class SequenceStore:
    """The raw series of one recorded sequence on the GPU + the recipe that turns window indices into engine inputs."""

    def __init__(self, arrays: Dict[str, np.ndarray], recipe: WindowRecipe, dtype: str = "bf16", device=None, fast: bool = True):
        if not torch.cuda.is_available():
            raise RuntimeError("window assembly runs on a HIP device; there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = eng.load_library()
        self.dtype = dtype
        self.torch_dtype = torch.bfloat16 if dtype == "bf16" else torch.float32      # the split plan ("x3") takes fp32 inputs
        self.names = recipe.series()
        self.series = []
        n_rows = None
        self._shared16 = {"series": [], "src": None}      # bf16 copies for the fused gather of Engine.step_mse_series (made on first use; shared with `transformed` siblings)
        for s in self.names:
            a = torch.as_tensor(np.asarray(arrays[s])).to(self.device, torch.float32)
            a = a.reshape(a.shape[0], -1).t()                       # column-major: one window of one column is contiguous
            n_rows = a.shape[1] if n_rows is None else min(n_rows, a.shape[1])
            pad = torch.zeros(a.shape[0], a.shape[1] + 8, dtype=torch.float32, device=self.device)     # 8 elements of slack behind every column
            pad[:, :a.shape[1]] = a                                 # (a 16-byte load of the fused gather may run past a window's last step)
            self.series.append(pad)
        self.n_rows = int(n_rows)
        if self.n_rows < recipe.history:
            raise ValueError("sequence shorter than one window")
        self._src = (C.c_void_p * len(self.series))(*[a.data_ptr() for a in self.series])
        self._pitch = (C.c_int64 * len(self.series))(*[a.shape[1] for a in self.series])     # column stride (rows + slack)
        self._rows = (C.c_int64 * len(self.series))(*[a.shape[1] - 8 for a in self.series])
        self._fast = bool(fast)
        self._describe(recipe)

    SIGN_FLAG = SIGN_FLAG

    def _describe(self, recipe: WindowRecipe, elements: Optional[Sequence[WindowRecipe]] = None) -> None:
        """The device tables, the descriptor and the per-store caches of `recipe` over the series already resident (the constructor; `transformed`).
        elements (`orbit`): the recipes of the K group elements, `recipe` the first of them -- their tables are stacked element-major."""
        self.recipe = recipe
        sidx = {s: i for i, s in enumerate(self.names)}
        ncols = {s: int(self.series[sidx[s]].shape[0]) for s in self.names}
        if elements is not None and len(elements) > 1:
            tabs = [r.tables(self.names, ncols) for r in elements]
            runs_k, rows, lab_k = stack_orbit_tables([t[:3] for t in tabs])
            self.n_elements = len(elements)
            runs, lab = runs_k[0], lab_k[0]
            all_runs, all_lab = [r for blk in runs_k for r in blk], [c for blk in lab_k for c in blk]
            signed = True      # (K > 1 implies sign_flags bit 0)
        else:
            runs, rows, lab, signed = recipe.tables(self.names, ncols)
            self.n_elements = 1
            all_runs, all_lab = runs, lab
        self.operators = [None]      # (`orbit` names its elements)
        self.element_recipes = list(elements) if elements is not None else [recipe]      # (symmetrise.OutputAction.from_store reads the elements' label tables)
        self.runs = torch.tensor(all_runs, dtype=torch.int32, device=self.device)
        self.rows = torch.tensor(rows, dtype=torch.int32, device=self.device)
        self.label_cols = torch.tensor(all_lab, dtype=torch.int32, device=self.device)
        d = eng.MshgnnWindowDesc()
        d.n_types = len(recipe.node_types); d.dtype = {"f32": 0, "bf16": 1, "x3": 2}[self.dtype]; d.history = recipe.history
        d.normalize = int(recipe.normalize)
        for i, t in enumerate(recipe.node_types):
            d.type_nodes[i] = recipe.num_nodes[t]; d.type_width[i] = recipe.width(t)
        d.n_src = len(self.series); d.n_runs = len(runs); d.runs = self.runs.data_ptr()
        d.fast_layout = int(self._fast)  # every row's runs are `history` long (or the single constant-1 run) and follow each other from feature 0
                                       # (fast=False: the general run-by-run gather kernel, kept for descriptors that do not promise this)
        d.n_rows = len(rows); d.rows = self.rows.data_ptr()
        d.n_label = len(recipe.label_cols); d.label_src = sidx[recipe.label_series] if recipe.label_series else 0
        d.label_rotate = int(recipe.label_rotate); d.quat_src = sidx[recipe.quat_series] if recipe.quat_series else -1
        d.label_cols = self.label_cols.data_ptr()
        d.sign_flags = 1 if signed else 0      # the tables carry sign flags (checked by the library on the first call, vouched for afterwards: bit 1)
        if self.n_elements > 1:
            d.sign_flags |= self.n_elements << 8      # K stacked element tables: a window's element rides in bits 56..63 of its start
        self.desc = d
        self._cache = {}
        self._run_ptrs = None
        self._eval_cache = {}
        self._stats_cache = {}
        if hasattr(self, "_run_ptrs_key"):
            del self._run_ptrs_key

    @property
    def series16(self):
        return self._shared16["series"]

    @property
    def _src16(self):
        return self._shared16["src"]

    def transformed(self, operator: str, group: GroupAction, mode: str = "MorphSym") -> "SequenceStore":
        """A sibling store of g . window (`WindowRecipe.transformed`) over THE SAME resident series: it shares the series tensors, their bf16 copies
        included, and owns only its runs, label tables, descriptor and caches -- no second copy of the data.  Every route that takes a store takes it."""
        recipe = self.recipe.transformed(operator, group, mode)
        # SHARED with the parent (by reference): device, lib, dtype, names, series, _shared16 (the bf16 copies), n_rows, _src / _pitch / _rows, _fast and a
        # ResidentDataset's seq_* lists.  OWNED by the sibling, all (re)made by _describe: recipe, runs, rows, label_cols, desc, _cache, _run_ptrs,
        # _run_ptrs_key, _eval_cache, _stats_cache, n_elements, operators.  A per-store attribute that depends on the recipe or is created lazily belongs in _describe.
        sib = object.__new__(type(self))
        sib.__dict__.update(self.__dict__)
        sib._describe(recipe)
        return sib

    def orbit(self, group: GroupAction, operators: Sequence[str] = ("gs", "gt", "gr"), mode: str = "MorphSym", identity: bool = True) -> "SequenceStore":
        """A sibling store whose batches carry a group element PER WINDOW: its tables stack the identity (identity=True) and each operator's
        `WindowRecipe.transformed`, element-major, over the same resident series (shared / owned exactly as in `transformed`).  `n_elements` is K,
        `operators` names the elements (None: the identity), `len()` is still the number of windows; `recipe` is element 0's.  `batch` / `assemble`
        take `elements`; a `DatasetView` of an orbit dataset has K * n indices."""
        recipes = self.recipe.orbit(group, operators, mode, identity)
        sib = object.__new__(type(self))
        sib.__dict__.update(self.__dict__)
        sib._describe(recipes[0], recipes)
        sib.operators = ([None] if identity else []) + list(operators)
        return sib

    def pack_starts(self, rows: torch.Tensor, elements) -> torch.Tensor:
        """Device start rows + one group element per window -> the packed starts an orbit descriptor's gathers take (element << 56 | row).  elements: a
        host sequence / tensor (range-checked here) or a device int tensor (trusted: the kernels clamp an index >= K to K - 1); None: element 0."""
        if elements is None:
            return rows
        el = elements if isinstance(elements, torch.Tensor) else torch.as_tensor(np.asarray(elements), dtype=torch.int64)
        el = el.flatten().to(torch.int64)
        if el.numel() != rows.numel():
            raise ValueError(f"{el.numel()} elements for {rows.numel()} windows")
        if not el.is_cuda:
            if int(el.min()) < 0 or int(el.max()) >= self.n_elements:
                raise IndexError(f"group element out of range [0, {self.n_elements})")
            if self.n_elements <= 1:
                return rows
            el = el.to(self.device, non_blocking=True)
        elif self.n_elements <= 1:
            raise ValueError("this store has one group element: device `elements` belong to an `orbit` store")
        return rows | (el << ELEMENT_SHIFT)

    def orbit_batch(self, rows, edge_index_dict) -> "WindowBatch":
        """The ORBIT-COMPLETE batch of the base windows `rows` of an `orbit` store: K * len(rows) windows in element-major order, window e * B + w = element e
        of base window rows[w] -- the order of `orbit_index_split` / ConcatDataset([ds, ds_gs, ...]) and what `symmetrise.orbit_average` takes.  rows: start
        rows, a host sequence / tensor (checked here) or a device int64 tensor (trusted, as in `WindowBatch`); the starts are packed on the device with
        torch integer ops on the current stream: capturable like `pack_starts`."""
        K = self.n_elements
        if K < 2:
            raise ValueError("orbit_batch needs an `orbit` store (this store has one group element)")
        st = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows), dtype=torch.int64)
        st = st.flatten().to(torch.int64)
        if st.numel() < 1:
            raise ValueError("no window indices")
        if not st.is_cuda:
            if int(st.min()) < 0 or int(st.max()) + self.recipe.history > self.n_rows:
                raise IndexError("window index out of range")
            st = st.to(self.device)
        el = torch.arange(K, dtype=torch.int64, device=st.device).repeat_interleave(st.numel())
        return WindowBatch(self, (st & ROW_MASK).repeat(K) | (el << ELEMENT_SHIFT), edge_index_dict)

    def __len__(self) -> int:
        """Number of windows (the reference's dataset length: rows - history + 1)."""
        return self.n_rows - self.recipe.history + 1

    def padded_width(self, t: str) -> int:
        return eng.row_pitch(self.recipe.width(t), 2 if self.dtype == "bf16" else 4)      # the engine's input layout

    def _buffers(self, B: int):
        """Output buffers for a batch of B windows, made once per batch size: the pad columns are zeroed here and never
        written again (the kernel only writes feature columns)."""
        if B not in self._cache:
            r = self.recipe
            xs = [torch.zeros(B * r.num_nodes[t], self.padded_width(t), dtype=self.torch_dtype, device=self.device) for t in r.node_types]
            y = torch.empty(B, len(r.label_cols), dtype=torch.float32, device=self.device) if r.label_cols else None
            q = torch.empty(B, 4, dtype=torch.float32, device=self.device) if r.quat_series else None
            self._cache = {B: (xs, y, q)}          # one batch size at a time
        return self._cache[B]

    def _stats_buffer(self, B: int) -> Optional[torch.Tensor]:
        """The statistics scratch of the standardised training steps (`Engine.step_mse_series_std` / `step_ce_series_std`) for a batch of B windows:
        `mshgnn_forward_series_stats_bytes` of fp64, made once per batch size (one batch size at a time, like `_buffers`); None for an
        unstandardised recipe (the library refuses it there)."""
        if B not in self._stats_cache:
            nbytes = int(self.lib.mshgnn_forward_series_stats_bytes(C.byref(self.desc), B))
            self._stats_cache = {B: torch.empty(nbytes // 8, dtype=torch.float64, device=self.device) if nbytes else None}
        return self._stats_cache[B]

    def assemble(self, starts, reuse_buffers: bool = False, elements=None) -> Tuple[List[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        """starts: window start rows (== the reference's dataset indices), a host sequence / tensor (checked on the host) or
        a device int64 tensor (trusted).  Returns (xs, y, r_o): xs[t] is [B * n_t, padded width] at the store's dtype --
        exactly what `Engine.forward` takes (pad columns are zero) --, y float32 [B, n_label], r_o float32 [B, 4].
        reuse_buffers=True returns the same tensors on every call of one batch size (a training loop that consumes the
        batch before asking for the next).  elements (an `orbit` store): one group element per window, a host sequence (range-checked) or a device
        int tensor (trusted); None: element 0, or whatever device `starts` already carry packed (`pack_starts`, a view's `starts`)."""
        r = self.recipe
        st = starts if isinstance(starts, torch.Tensor) else torch.as_tensor(np.asarray(starts), dtype=torch.int64)
        st = st.flatten().to(torch.int64)
        if st.numel() < 1:
            raise ValueError("no window indices")
        if not st.is_cuda:
            if int(st.min()) < 0 or int(st.max()) + r.history > self.n_rows:
                raise IndexError("window index out of range")
            st = st.to(self.device, non_blocking=True)
        st = self.pack_starts(st, elements)
        B = st.numel()
        if reuse_buffers:
            xs, y, q = self._buffers(B)
        else:
            xs = [torch.zeros(B * r.num_nodes[t], self.padded_width(t), dtype=self.torch_dtype, device=self.device) for t in r.node_types]
            y = torch.empty(B, len(r.label_cols), dtype=torch.float32, device=self.device) if r.label_cols else None
            q = torch.empty(B, 4, dtype=torch.float32, device=self.device) if r.quat_series else None
        xp = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        pitch = (C.c_int64 * len(xs))(*[x.shape[1] for x in xs])
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self.lib.mshgnn_assemble_windows(C.byref(self.desc), self._src, self._pitch, self._rows, st.data_ptr(), B, xp, pitch,
                                              y.data_ptr() if y is not None else None, q.data_ptr() if q is not None else None, stream)
        eng._check(self.lib, rc, "mshgnn_assemble_windows")
        if self.desc.sign_flags & 3 == 1:
            self.desc.sign_flags |= 2     # the library has checked these tables: later calls vouch for them (no table read-back per call)
        return xs, y, q

    def batch(self, starts, edge_index_dict, elements=None) -> "WindowBatch":
        """A minibatch of window indices shaped like the PyG batch the wrappers take (see WindowBatch); elements: as in `assemble`."""
        return WindowBatch(self, starts, edge_index_dict, elements)

    def eval_buffers(self, B: int, labels: bool = True, n_flags: int = 0):
        """The by-product buffers and the statistics scratch of `Engine.forward_series` for a batch of B windows, made once per batch size (one batch
        size at a time, like `_buffers`): (y, quat, labels_int, stats).  labels=False or a recipe without labels (a test sequence): no y / quat /
        labels_int.  labels_int (int32 contact flags) only when the recipe has one unrotated label per flag (n_flags = the model's out nodes).
        stats: `mshgnn_forward_series_stats_bytes` of scratch for standardised recipes, else None."""
        r = self.recipe
        want = bool(labels and r.label_cols)
        key = (B, want, n_flags)
        if key not in self._eval_cache:
            y = torch.empty(B, len(r.label_cols), dtype=torch.float32, device=self.device) if want else None
            q = torch.empty(B, 4, dtype=torch.float32, device=self.device) if want and r.quat_series else None
            li = torch.empty(B, n_flags, dtype=torch.int32, device=self.device) if want and n_flags and len(r.label_cols) == n_flags and not r.label_rotate else None
            nbytes = int(self.lib.mshgnn_forward_series_stats_bytes(C.byref(self.desc), B))
            stats = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device) if nbytes else None
            self._eval_cache = {key: (y, q, li, stats)}
        return self._eval_cache[key]

    def series_step_args(self, bf16: bool = True):
        """What Engine.step_mse_series hands to mshgnn_step_mse_series: bf16 copies of the series (same strides; bf16=False, the split plan:
        none -- it gathers from the fp32 series themselves) and the run-pointer scratch."""
        if self._run_ptrs is None:
            self._run_ptrs = torch.zeros(max(1, self.n_elements * int(self.desc.n_runs)), dtype=torch.int64, device=self.device)      # (every element's block)
        if bf16 and self._src16 is None:
            self._shared16["series"] = [a.to(torch.bfloat16) for a in self.series]
            self._shared16["src"] = (C.c_void_p * len(self.series16))(*[a.data_ptr() for a in self.series16])
        return (self._src16 if bf16 else None), self._run_ptrs


class WindowBatch:
    """One minibatch of window indices of a `SequenceStore`, with the attributes the reference's wrappers read off a PyG batch
    (`x_dict`, `edge_index_dict`, `y`, `r_o`, `batch_size`; gnnLightning.py:680-722).  Nothing is gathered when it is made: a wrapper's
    `training_step` hands the indices to the engine, whose encoder gathers its inputs from the resident series
    (`models.fused_training_step_windows` -> `mshgnn_step_mse_series` / `mshgnn_step_ce_series`, standardised recipes: their `_std` forms) and leaves the labels here; the evaluation steps
    under torch.no_grad() do the same without materialising anything (`models.forward_windows` -> `mshgnn_forward_series`); any other consumer
    (the two-call route, a model the fused routes do not take) gets the windows assembled on first access (`SequenceStore.assemble`, the store's reusable buffers:
    consume a batch before asking the store for the next one).

    Start rows given as a DEVICE tensor are not checked (see the constructor); indices that a sampler produces on the device go through a
    `ResidentDataset` view (`DatasetView.batch`), whose mapping kernel bounds every one of them -- one sequence is a dataset of one."""

    def __init__(self, store: SequenceStore, starts, edge_index_dict, elements=None):
        st = starts if isinstance(starts, torch.Tensor) else torch.as_tensor(np.asarray(starts), dtype=torch.int64)
        st = st.flatten().to(torch.int64)
        # Contract: every start index i satisfies 0 <= i and i + history <= store.n_rows (the fused-gather kernels read the series at
        # [i, i + history) without a bound check).  Host indices are checked here; DEVICE start rows are taken as they are, because checking them costs a
        # host synchronisation per batch -- `store.check_starts = True` turns that check on (debugging a sampler).  The CHECKED route for indices made on
        # the device is a `ResidentDataset` view: `view.batch(device_indices, ...)` maps dataset indices to start rows with `mshgnn_dataset_starts`, which
        # sends every index outside the view to row 0 (always a whole window) and raises a flag that `view.check()` reads once per epoch.
        # An `orbit` store: `elements` gives one group element per window (host values range-checked, device values trusted) and `starts` keeps the packed
        # words element << 56 | row that every route hands to the library; device starts may arrive packed already (a view's `starts`).
        if not st.is_cuda or getattr(store, "check_starts", False):
            rows = st & ROW_MASK if st.is_cuda and store.n_elements > 1 else st
            if st.numel() < 1 or int(rows.min()) < 0 or int(rows.max()) + store.recipe.history > store.n_rows:
                raise IndexError("window index out of range")
            st = st.to(store.device)
        st = store.pack_starts(st, elements)
        self.store, self.starts, self.edge_index_dict = store, st, edge_index_dict
        self.batch_size = int(st.numel())
        self._x = self._y = self._q = None

    def _assemble(self):
        if self._x is None:
            xs, y, q = self.store.assemble(self.starts, reuse_buffers=True)
            self._x = dict(zip(self.store.recipe.node_types, xs))
            self._y = y if self._y is None else self._y
            self._q = q if self._q is None else self._q

    def _labels_from_step(self, xs, y, q):
        """(the fused training step materialised the windows and the labels as a by-product)"""
        self._x = dict(zip(self.store.recipe.node_types, xs)) if xs is not None else None
        self._y, self._q = y, q

    @property
    def elements(self) -> Optional[torch.Tensor]:
        """The group element of every window (device int64 [B]) of an `orbit` store's batch, as the packed starts carry it; None for any other store."""
        return (self.starts >> ELEMENT_SHIFT) if self.store.n_elements > 1 else None

    @property
    def x_dict(self):
        self._assemble()
        return self._x

    @property
    def y(self):
        if self._y is None:
            self._assemble()
        return self._y

    @property
    def r_o(self):
        if self._q is None:
            self._assemble()
        return self._q


# --- a resident dataset of several sequences ------------------------------------------------------------------------------------------------------
# The reference's scripts never train on one sequence: research/train_regression-grf_msgn.py:57-73 cuts each of eight sequences at
# int(np.round((len - 1) * 0.85)) into a training and a validation Subset, joins them with ConcatDataset and shuffles minibatches across all of them.
# Here the sequences' series are concatenated row-wise into ONE SequenceStore and a dataset index becomes a start row of the concatenated series
# (host: `dataset_index_map` / `dataset_lookup`; device: mshgnn_dataset_starts), so every route that takes a store runs unchanged.

def dataset_window_counts(lengths: Sequence[int], history: int) -> List[int]:
    """Windows per sequence (rows - history + 1: the reference's dataset length); a sequence shorter than one window is refused, naming its position."""
    for s, n in enumerate(lengths):
        if int(n) < history:
            raise ValueError(f"sequence {s} has {int(n)} rows: shorter than one window of {history} steps")
    return [int(n) - history + 1 for n in lengths]


def dataset_split_ranges(lengths: Sequence[int], history: int, fraction: float = 0.85, drop_last: bool = True) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """The training and validation window ranges of the reference's scripts, per sequence (train_regression-grf_msgn.py:63-67): with len_s windows,
    m = len_s - 1 (drop_last: "dynamics models can't use the last entry") or len_s, k = int(np.round(m * fraction)) -- numpy's round-half-even on the
    float product --, train = [0, k), val = [k, m)."""
    train, val = [], []
    for n in dataset_window_counts(lengths, history):
        m = n - 1 if drop_last else n
        k = min(max(int(np.round(m * fraction)), 0), m)
        train.append((0, k)); val.append((k, m))
    return train, val


def dataset_index_map(lengths: Sequence[int], history: int, ranges: Optional[Sequence[Tuple[int, int]]] = None) -> Tuple[List[int], List[int]]:
    """(cum, first_row) of a view of a dataset whose sequences have `lengths` rows: sequence s contributes its windows [lo_s, hi_s) (`ranges`; None: all of
    them, an empty range is allowed), in sequence order.  cum[s] .. cum[s + 1] are the view's indices that fall into sequence s (cum has one entry more
    than there are sequences, cum[0] == 0), first_row[s] the row of the CONCATENATED series at which window lo_s of sequence s starts.  Index i with
    cum[s] <= i < cum[s + 1] is the window that starts at first_row[s] + (i - cum[s]) -- what `ConcatDataset([Subset(d_s, arange(lo_s, hi_s))])[i]` is.
    No window straddles two sequences: hi_s <= rows_s - history + 1."""
    counts = dataset_window_counts(lengths, history)
    if ranges is None:
        ranges = [(0, n) for n in counts]
    if len(ranges) != len(counts):
        raise ValueError(f"{len(ranges)} ranges for {len(counts)} sequences")
    cum, first_row, row0 = [0], [], 0
    for s, ((lo, hi), n) in enumerate(zip(ranges, counts)):
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"range [{lo}, {hi}) of sequence {s} is outside its {n} windows")
        cum.append(cum[-1] + hi - lo)
        first_row.append(row0 + lo)
        row0 += int(lengths[s])
    return cum, first_row


def dataset_lookup(cum: Sequence[int], first_row: Sequence[int], index: int) -> int:
    """The start row of dataset index `index` (the host mirror of one thread of mshgnn_dataset_starts); IndexError outside [0, cum[-1])."""
    i = int(index)
    if not 0 <= i < cum[-1]:
        raise IndexError(f"dataset index {i} out of range [0, {cum[-1]})")
    lo, hi = 0, len(cum) - 1          # cum[lo] <= i < cum[hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cum[mid] <= i:
            lo = mid
        else:
            hi = mid
    return first_row[lo] + (i - cum[lo])


class ResidentDataset(SequenceStore):
    """Several recorded sequences on the GPU as ONE `SequenceStore`: every named series is the row-wise concatenation of the sequences' series (column-major,
    8 elements of slack behind every column as before -- a 16-byte load that runs past a window's last step lands in the next sequence's rows, whose
    elements are cut or discarded like the slack's; only the last sequence relies on the slack).  Everything that takes a store takes this one and launches
    the same kernels (`assemble`, the fused training and evaluation routes, `wrappers.evaluate_sequence`): their `starts` are rows of the concatenated
    series.

    Dataset indices are the reference's: sequence s with n_s rows has n_s - history + 1 windows, index i of sequence s starts at row i of that sequence,
    no window straddles two sequences, `len(dataset)` is the sum.  `view()`, `subset(ranges)` and `split()` give `DatasetView`s that map indices to start
    rows, on the host for host indices and with `mshgnn_dataset_starts` for device indices."""

    def __init__(self, sequences: List[Dict[str, np.ndarray]], recipe: WindowRecipe, dtype: str = "bf16", device=None, fast: bool = True,
                 names: Optional[Sequence[str]] = None):
        if len(sequences) < 1:
            raise ValueError("a dataset needs at least one sequence")
        if names is not None and len(names) != len(sequences):
            raise ValueError(f"{len(names)} names for {len(sequences)} sequences")
        seq_names = [str(x) for x in names] if names is not None else [f"seq{k}" for k in range(len(sequences))]
        names = recipe.series()
        lengths, cols, parts = [], None, {s: [] for s in names}
        for k, seq in enumerate(sequences):
            arrs = {}
            for s in names:
                a = np.asarray(seq[s])
                arrs[s] = a.reshape(a.shape[0], -1)
            n = min(a.shape[0] for a in arrs.values())          # (a store's rows: the shortest of its series)
            if n < recipe.history:
                raise ValueError(f"sequence {k} has {n} rows: shorter than one window of {recipe.history} steps")
            c = {s: a.shape[1] for s, a in arrs.items()}
            if cols is None:
                cols = c
            elif c != cols:
                bad = [s for s in names if c[s] != cols[s]]
                raise ValueError(f"sequence {k}: series {bad} have {[c[s] for s in bad]} columns, sequence 0 has {[cols[s] for s in bad]}")
            lengths.append(int(n))
            for s in names:
                parts[s].append(arrs[s][:n])
        super().__init__({s: np.concatenate(parts[s], 0) for s in names}, recipe, dtype=dtype, device=device, fast=fast)
        self.seq_rows = lengths
        self.seq_windows = dataset_window_counts(lengths, recipe.history)
        self.seq_first_row = [int(x) for x in np.concatenate([[0], np.cumsum(lengths)[:-1]])]
        self.seq_names = seq_names      # (`names`: the sequences' names, default "seq0", ...; a view carries them -- an evaluation table's column groups)

    def __len__(self) -> int:
        """Number of windows: the sum over the sequences (fewer than rows - history + 1 of the concatenated series: nothing straddles)."""
        return sum(self.seq_windows)

    def subset(self, ranges: Sequence[Tuple[int, int]]) -> "DatasetView":
        """The windows [lo_s, hi_s) of every sequence s, concatenated in sequence order; an empty range is allowed."""
        return DatasetView(self, ranges)

    def view(self) -> "DatasetView":
        """Every window of every sequence."""
        return DatasetView(self, [(0, n) for n in self.seq_windows])

    def split(self, fraction: float = 0.85, drop_last: bool = True) -> Tuple["DatasetView", "DatasetView"]:
        """(train, val) views with the scripts' arithmetic per sequence (`dataset_split_ranges`)."""
        train, val = dataset_split_ranges(self.seq_rows, self.recipe.history, fraction, drop_last)
        return DatasetView(self, train), DatasetView(self, val)


class DatasetView:
    """A range of windows per sequence of a `ResidentDataset`, indexed 0 .. len(view) - 1 in sequence order like the reference's
    `ConcatDataset` of `Subset`s.  Host indices are checked and mapped on the host; device indices are mapped by `mshgnn_dataset_starts`, which
    writes start row 0 for an index outside the view and sets the view's `bad` word -- no host synchronisation per batch; `check()` reads the word."""

    def __init__(self, dataset: ResidentDataset, ranges: Sequence[Tuple[int, int]]):
        self.dataset = dataset
        self.ranges = [(int(lo), int(hi)) for lo, hi in ranges]
        self.cum, self.first_row = dataset_index_map(dataset.seq_rows, dataset.recipe.history, self.ranges)
        dev = dataset.device
        self._cum_np, self._first_np = np.asarray(self.cum, dtype=np.int64), np.asarray(self.first_row, dtype=np.int64)
        self._cum = torch.from_numpy(self._cum_np).to(dev)
        self._first = torch.from_numpy(self._first_np).to(dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)      # set by the mapping kernel, zeroed by check(): accumulates over an epoch
        # an `orbit` dataset: K * n indices over the view's n windows, index i = element i // n of window i % n -- ConcatDataset([view, view_gs, view_gt, view_gr])
        self.n_elements = int(getattr(dataset, "n_elements", 1))
        self.n_windows = int(self.cum[-1])

    def __len__(self) -> int:
        return self.n_elements * self.n_windows

    # segment ids of an evaluation table (metrics.SegmentedMetrics): one row per group element, one column per sequence
    @property
    def n_sequences(self) -> int:
        return len(self.first_row)

    @property
    def names(self) -> List[str]:
        return list(self.dataset.seq_names)

    @property
    def segment_shape(self) -> Tuple[int, int]:
        return self.n_elements, self.n_sequences

    @property
    def n_segments(self) -> int:
        return self.n_elements * self.n_sequences

    def segments(self, indices, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Segment ids (device int32) element * n_sequences + sequence of the view's `indices`.  A host sequence / tensor is checked here (IndexError) and
        mapped on the host; a device integer tensor is mapped with torch.searchsorted over the view's device `cum` and the integer ops `starts` uses for
        the element split -- on the device, capturable, no synchronisation --, an index outside [0, K n) to -1 (`SegmentedMetrics` counts it in its
        overflow row).  A sequence whose range is empty owns no index and so no id.  out: an int32 tensor on the dataset's device, of the same size, to write into."""
        K, n, S = self.n_elements, self.n_windows, self.n_sequences
        dev = self.dataset.device
        ix = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int64)
        if ix.numel() < 1:
            raise ValueError("no window indices")
        if not ix.is_cuda:
            ix = ix.flatten().to(torch.int64).numpy()
            if int(ix.min()) < 0 or int(ix.max()) >= len(self):
                raise IndexError(f"dataset index out of range [0, {len(self)})")
            el = ix // n
            seg = torch.from_numpy((el * S + (np.searchsorted(self._cum_np, ix - el * n, side="right") - 1)).astype(np.int32)).to(dev)
        else:
            ix = ix.reshape(-1).to(torch.int64)
            valid = (ix >= 0) & (ix < K * n)
            el = torch.div(ix, max(n, 1), rounding_mode="floor")
            seq = torch.searchsorted(self._cum, (ix - el * n).contiguous(), right=True) - 1
            seg = torch.where(valid, el * S + seq, torch.full_like(ix, -1))
        if out is None:
            return seg.to(torch.int32)
        if out.device != seg.device or out.dtype != torch.int32 or out.numel() != seg.numel() or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 tensor on the dataset's device with one element per index")
        out.view(-1).copy_(seg)
        return out

    def starts(self, indices, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Start rows (device int64, rows of the dataset's concatenated series) of the view's `indices`.  A host sequence / tensor is checked here
        (IndexError) and mapped on the host; a device int64 tensor goes through mshgnn_dataset_starts on the current stream (`out`: a device int64
        tensor of the same size to write into -- a captured step's static buffer).  An `orbit` dataset: index i is element i // n of window i % n and
        the result are PACKED starts (element << 56 | row); the split is made with torch integer ops around the mapping kernel, on the device and
        capturable, and an index outside [0, K n) reaches the kernel as -1: row 0, element 0, and the `bad` word is set."""
        ds = self.dataset
        K, n = self.n_elements, self.n_windows
        ix = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int64)
        if ix.numel() < 1:
            raise ValueError("no window indices")
        if not ix.is_cuda:
            ix = ix.flatten().to(torch.int64).numpy()
            if int(ix.min()) < 0 or int(ix.max()) >= len(self):
                raise IndexError(f"dataset index out of range [0, {len(self)})")
            el = ix // n if K > 1 else None
            if K > 1:
                ix = ix - el * n
            s = np.searchsorted(self._cum_np, ix, side="right") - 1
            rows = self._first_np[s] + (ix - self._cum_np[s])
            st = torch.from_numpy(rows | (el << ELEMENT_SHIFT) if K > 1 else rows).to(ds.device)
            if out is not None:
                out.copy_(st)
                return out
            return st
        if ix.dtype != torch.int64 or not ix.is_contiguous():
            ix = ix.to(torch.int64).contiguous()
        ix = ix.view(-1)
        el = None
        if K > 1:
            valid = (ix >= 0) & (ix < K * n)
            el = torch.where(valid, torch.div(ix, max(n, 1), rounding_mode="floor"), torch.zeros_like(ix))
            ix = torch.where(valid, ix - el * n, torch.full_like(ix, -1))
        if out is None:
            out = torch.empty_like(ix)
        elif not out.is_cuda or out.dtype != torch.int64 or out.numel() != ix.numel() or not out.is_contiguous():
            raise ValueError("out must be a contiguous device int64 tensor with one element per index")
        if not hasattr(ds.lib, "mshgnn_dataset_starts"):
            raise eng.MshgnnError("this build of the library has no mshgnn_dataset_starts")
        with torch.cuda.device(ds.device):
            rc = ds.lib.mshgnn_dataset_starts(self._cum.data_ptr(), self._first.data_ptr(), len(self.first_row), ix.data_ptr(), ix.numel(), out.data_ptr(),
                                              self.bad.data_ptr(), C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream))
        eng._check(ds.lib, rc, "mshgnn_dataset_starts")
        if el is not None:
            out.bitwise_or_(el << ELEMENT_SHIFT)
        return out

    def check(self) -> None:
        """One host synchronisation: IndexError if a device index mapped since the last check was outside the view (the flag is cleared)."""
        if int(self.bad.item()) != 0:
            self.bad.zero_()
            raise IndexError(f"a device index given to this view was outside [0, {len(self)}): its window was replaced by the view's row 0")

    def batch(self, indices, edge_index_dict) -> WindowBatch:
        """An ordinary `WindowBatch` of the dataset whose `starts` are the mapped rows; `indices` (as given, on the device) stays on it."""
        st = self.starts(indices)
        wb = WindowBatch(self.dataset, st, edge_index_dict)
        ix = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int64)
        wb.indices = ix.reshape(-1).to(st.device, torch.int64)
        return wb

    def orbit_batch(self, indices, edge_index_dict) -> WindowBatch:
        """The ORBIT-COMPLETE batch (`SequenceStore.orbit_batch`) of the BASE windows `indices` in [0, n_windows) of a view of an `orbit` dataset: the view's
        indices e * n_windows + indices[w], element-major, through `batch`.  Host indices are checked here; a device index outside [0, n_windows) reaches
        the mapping kernel as -1 under every element (row 0, element 0, the `bad` word is set)."""
        K, n = self.n_elements, self.n_windows
        if K < 2:
            raise ValueError("orbit_batch needs a view of an `orbit` dataset (this dataset has one group element)")
        ix = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int64)
        ix = ix.reshape(-1).to(torch.int64)
        if ix.numel() < 1:
            raise ValueError("no window indices")
        if not ix.is_cuda:
            if int(ix.min()) < 0 or int(ix.max()) >= n:
                raise IndexError(f"base window index out of range [0, {n})")
            ix = ix.to(self.dataset.device)
        off = torch.arange(K, dtype=torch.int64, device=ix.device).repeat_interleave(ix.numel()) * n
        rep = ix.repeat(K)
        return self.batch(torch.where((rep >= 0) & (rep < n), rep + off, torch.full_like(rep, -1)), edge_index_dict)

    def epoch(self, batch_size: int, generator: Optional[torch.Generator] = None, shuffle: bool = True, drop_last: bool = False):
        """Device index tensors of one pass over the view: ONE torch.randperm per epoch (on the device; with a host generator it is drawn on the host
        and copied once), then slices of it -- no host round trip per batch.  When the generator is exhausted, `check()` runs once."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        n, dev = len(self), self.dataset.device
        if not shuffle:
            order = torch.arange(n, dtype=torch.int64, device=dev)
        elif generator is not None and generator.device.type == "cpu":
            order = torch.randperm(n, generator=generator).to(dev)
        else:
            order = torch.randperm(n, generator=generator, device=dev)
        stop = n - n % batch_size if drop_last else n
        for lo in range(0, stop, batch_size):
            yield order[lo:lo + batch_size]
        self.check()
