"""Generator of tests/golden/windows_mlp.npz -- runs ONLY where the reference checkout is present (the build container); nothing of the reference ships.

The reference's own `FlexibleDataset.get_helper_mlp` (datasets_py/flexibleDataset.py:510-535) and `load_data_sorted` (:336-400) are run on a stub dataset
that carries a small deterministic synthetic A1 sequence, the way oracle/gen_window_golden.py runs the graph datasets' helpers.  The fixture holds data
only: the raw series, the joint / foot orders, a handful of window indices and, per index, the x and y the reference returns, without and with
`normalize`.  tests/test_mlp.py evaluates `windows.quadsdk_a1_mlp_recipe`'s tables on the host against it."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_window_golden as gw  # noqa: E402  (the import stand-ins, the synthetic sequence, the joint / foot orders)

T, N, SEED = 30, 80, 20250301
STARTS = [0, 1, 17, N - T]


def stub(qmod, fmod, seq, normalize):
    s = types.SimpleNamespace()
    s.mat_data = seq; s.history_length = T; s.grf_dimension = 1; s.grf_body_to_world_frame = False
    s.normalize = normalize; s.symmetry_operator = None
    s.joint_node_indices_sorted = gw.JOINT_PERM; s.foot_node_indices_sorted = gw.FOOT_PERM
    s.variables_to_use_all = np.array([0, 1, 2, 3, 4])      # lin_acc, ang_vel, j_p, j_v, j_T (the A1 dataset has no foot positions / velocities)
    s.load_data_at_dataset_seq_3d = types.MethodType(qmod.QuadSDKDataset_A1.load_data_at_dataset_seq_3d, s)
    s.load_data_at_dataset_seq = types.MethodType(qmod.QuadSDKDataset_A1.load_data_at_dataset_seq, s)
    s.load_data_sorted = types.MethodType(fmod.FlexibleDataset.load_data_sorted, s)
    s.get = types.MethodType(fmod.FlexibleDataset.get_helper_mlp, s)
    return s


def main():
    qmod = gw.reference_module()
    fmod = importlib.import_module("ms_hgnn.datasets_py.flexibleDataset")
    seq = gw.synthetic_sequence(SEED, N)
    fx = {"T": np.array(T), "N": np.array(N), "starts": np.array(STARTS), "joint_perm": gw.JOINT_PERM.astype(np.int64),
          "foot_perm": gw.FOOT_PERM.astype(np.int64)}
    for k in ("imu_acc", "imu_omega", "q", "qd", "tau", "F", "r_o"):
        fx["series:" + k] = np.asarray(seq[k], dtype=np.float64)
    # numpy 2 refuses np.nan_to_num(copy=False) on the torch tensor the reference hands it (flexibleDataset.py:396); numpy 1.x converted it first -- the same
    # one-function shim as oracle/gen_window_golden.py, in this generator only
    orig = np.nan_to_num
    np.nan_to_num = lambda x, copy=True, nan=0.0, posinf=None, neginf=None: orig(x if isinstance(x, np.ndarray) else np.asarray(x), copy=copy, nan=nan,
                                                                                  posinf=posinf, neginf=neginf)
    try:
        for norm in (False, True):
            ds = stub(qmod, fmod, seq, norm)
            for st in STARTS:
                x, y = ds.get(st)
                fx[f"{'norm' if norm else 'raw'}:{st}:x"] = x.numpy().astype(np.float64)
                fx[f"{'norm' if norm else 'raw'}:{st}:y"] = y.numpy().astype(np.float64)
    finally:
        np.nan_to_num = orig
    out = os.path.join(ROOT, "tests", "golden", "windows_mlp.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes;", "x:", fx[f"raw:{STARTS[0]}:x"].shape, "y:", fx[f"raw:{STARTS[0]}:y"].shape)


if __name__ == "__main__":
    main()
