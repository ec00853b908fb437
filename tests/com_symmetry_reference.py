"""The action of the Solo symmetry groups (cfg/solo-k4.yaml, cfg/solo-c2.yaml) on a centroidal-momentum window, in numpy straight from the yaml tables
-- not through morphsym_hgnn_amd.windows: every sorted part X [T, n] becomes X'[:, k] = c[k] X[:, P[k]] over its flat index k = node * n_axes + axis,
gs = (P0, c0), gt = (P1, c1), gr = (P0[P1[k]], c0 c1):

  * q, qd [T, 12] in graph (sorted) joint order by the `js` tables;
  * the base series, tiled to the n_base base nodes, [T, 3 n_base] by `permutation_Q_bs` with `reflection_Q_bs_lin` / `reflection_Q_bs_ang`;
  * the labels [n_base][lin(3) | ang(3)]: the lin halves of all base nodes are one vector [3 n_base] acted on like the linear base series, the ang halves
    like the angular one.

One base node (S4, COM_HGNN, the MLP's 6 labels) against tables tiled over 2 or 4 nodes holds ONE copy: that copy's reflection, no permutation.
`window` lays the result out as the window gathers do (per node the T steps of every column contiguous, variable-major)."""
import os

import numpy as np
import yaml

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "morphsym_hgnn_amd", "cfg")
OPS = ("gs", "gt", "gr")
KINDS = {"k4": ("k4_com", 4, "solo-k4"), "c2": ("c2_com", 2, "solo-c2"), "s4": ("s4_com", 1, "solo-k4"), "mlp": (None, 1, "solo-k4")}      # recipe kind, n_base, group file


def load(name):
    with open(os.path.join(CFG, name + ".yaml")) as f:
        return yaml.safe_load(f)


def table(group, part, op, n_base=None):
    """(P, c) of part "js" | "bs_lin" | "bs_ang" for op None (identity) | "gs" | "gt" | "gr"; n_base = 1: the one-copy rule."""
    (P0, P1), (c0, c1) = group["permutation_Q_" + ("js" if part == "js" else "bs")], group["reflection_Q_" + part]
    P0, P1, c0, c1 = (np.asarray(a, dtype=np.int64) for a in (P0, P1, c0, c1))
    if op is None:
        P, c = np.arange(len(P0)), np.ones(len(P0), dtype=np.int64)
    elif op == "gs":
        P, c = P0, c0
    elif op == "gt":
        P, c = P1, c1
    else:
        assert op == "gr"
        P, c = P0[P1], c0 * c1
    if part != "js" and n_base == 1 and len(P) > 3:
        assert (c.reshape(-1, 3) == c[:3]).all() and (P % 3 == np.arange(len(P)) % 3).all()      # the tables ARE tiled copies
        P, c = np.arange(3), c[:3]
    return P, c


def act(X, P, c):
    """X'[..., k] = c[k] X[..., P[k]]"""
    return np.asarray(X)[..., P] * c


def labels(group, op, y6, n_base):
    """g . labels of one window: y6 [6] = the row of Y, tiled to the base nodes -> [6 n_base]"""
    y = np.tile(np.asarray(y6, dtype=np.float64), n_base).reshape(n_base, 6)
    lin = act(y[:, :3].reshape(-1), *table(group, "bs_lin", op, n_base)).reshape(n_base, 3)
    ang = act(y[:, 3:].reshape(-1), *table(group, "bs_ang", op, n_base)).reshape(n_base, 3)
    return np.concatenate([lin, ang], 1).reshape(-1)


def output_action(group, ops, n_base):
    """(perm, sign) [1 + len(ops)][6 n_base] with y_e[k] = sign[e][k] y[perm[e][k]], element 0 the identity: the label action applied to the slot numbers"""
    perm, sign = [], []
    for op in (None,) + tuple(ops):
        idx = np.arange(6 * n_base).reshape(n_base, 6)
        p = np.empty((n_base, 6), dtype=np.int64)
        s = np.empty((n_base, 6), dtype=np.int64)
        for half, part in ((slice(0, 3), "bs_lin"), (slice(3, 6), "bs_ang")):
            P, c = table(group, part, op, n_base)
            p[:, half] = idx[:, half].reshape(-1)[P].reshape(n_base, 3)
            s[:, half] = c.reshape(n_base, 3)
        perm.append(p.reshape(-1).tolist()); sign.append(s.reshape(-1).tolist())
    return perm, sign


def window(group, op, kind, seq, start, T, joint_perm):
    """({type: [n_nodes, width]}, labels [6 n_base]) of g . window at `start` in fp64; kind: a key of KINDS; seq: the series of `solo_com_arrays`."""
    nb = KINDS[kind][1]
    jp = np.asarray(joint_perm, dtype=np.int64)
    rows = slice(start, start + T)
    f = lambda s: np.asarray(seq[s], dtype=np.float64)
    q, qd = (act(f(s)[rows][:, jp], *table(group, "js", op)) for s in ("q", "qd"))                                      # [T, 12]
    if kind == "mlp":
        xs = {"mlp": np.concatenate([q.T.reshape(-1), qd.T.reshape(-1)])[None, :]}
    else:
        lin = act(np.tile(f("base_lin")[rows], (1, nb)), *table(group, "bs_lin", op, nb))                              # [T, 3 nb]
        ang = act(np.tile(f("base_ang")[rows], (1, nb)), *table(group, "bs_ang", op, nb))
        xs = {"base": np.stack([np.concatenate([lin[:, 3 * n:3 * n + 3].T.reshape(-1), ang[:, 3 * n:3 * n + 3].T.reshape(-1)]) for n in range(nb)]),
              "joint": np.stack([np.concatenate([q[:, j], qd[:, j]]) for j in range(12)])}
    return xs, labels(group, op, f("Y")[start + T - 1], nb)
