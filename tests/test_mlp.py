"""CPU: the MLP baselines without a device -- `windows.mlp_recipe` tables against the reference's own get_helper_mlp (tests/golden/windows_mlp.npz, made by
tools/gen_mlp_window_golden.py), the flat parameter layout against torch's state_dict order, the descriptor refusals of mshgnn_mlp_compile_host, the
wrappers' constructor and attribute names, the checkpoint round trip and the missing CPU fallback."""
import inspect
import os

import numpy as np
import pytest
import torch
from torch import nn

from morphsym_hgnn_amd import checkpoint, engine, models, windows, wrappers
from tests import mlp_reference as mr
from tests import test_window_symmetry as ws

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "windows_mlp.npz"))


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
def test_mlp_recipe_reproduces_get_helper_mlp(normalize):
    T = int(FX["T"])
    seq = {k[len("series:"):]: FX[k] for k in FX.files if k.startswith("series:")}
    recipe = windows.quadsdk_a1_mlp_recipe(FX["joint_perm"].astype(int), FX["foot_perm"].astype(int), T, 1, normalize=normalize)
    assert recipe.node_types == ["mlp"] and recipe.num_nodes == {"mlp": 1} and recipe.width("mlp") == T * 42
    runs, rows, lab, signed = recipe.tables()
    assert len(runs) == 42 and rows == [[0, 42]] and not signed and [r[2] for r in runs] == [T * i for i in range(42)] and all(r[4] == T for r in runs)
    for st in FX["starts"]:
        xs, y = ws.evaluate(recipe, seq, int(st))
        x = xs["mlp"].reshape(-1)
        want_x, want_y = FX[f"{'norm' if normalize else 'raw'}:{int(st)}:x"], FX[f"{'norm' if normalize else 'raw'}:{int(st)}:y"]
        assert x.shape == want_x.shape and np.abs(x - want_x).max() <= (1e-12 * np.abs(want_x).max() if normalize else 0.0), int(st)
        assert np.array_equal(np.asarray(y).reshape(-1), want_y.reshape(-1))


def test_mlp_recipes_of_the_three_datasets():
    mc = windows.minicheetah_mlp_recipe(ws.JP, ws.FP, 150)
    assert mc.width("mlp") == 8100 and len(mc.tables()[0]) == 54 and mc.label_series == "contacts" and len(mc.label_cols) == 4
    assert [s for s, _ in mc.variables["mlp"]] == ["imu_acc", "imu_omega", "q", "qd", "p", "v"]
    a1 = windows.quadsdk_a1_mlp_recipe(ws.JP, ws.FP, 150)
    assert a1.width("mlp") == 6300 and a1.label_cols == windows.quadsdk_a1_c2_recipe(ws.JP, ws.FP, 150).label_cols
    solo = windows.solo_com_mlp_recipe(list(range(12)))
    assert solo.width("mlp") == 24 and solo.label_cols == [0, 1, 2, 3, 4, 5]
    # absent variables are skipped; the transformed recipes act on the single base copy with its reflection alone
    assert windows.mlp_recipe([("a", [0, 1]), (None, []), ("b", [])], 5).width("mlp") == 10
    gs = mc.transformed("gs", ws.K4)
    assert gs.variables["mlp"][0][1] == [[0, 1, 2]] and gs.variable_signs["mlp"][0] == [list(ws.K4.reflection["bs_lin"][0][:3])]
    assert len(mc.orbit(ws.K4)) == 4


@pytest.mark.parametrize("L", [2, 3, 8])
def test_flat_layout_is_torchs_state_dict_order(L):
    info = engine.mlp_compile_host(450, 128, 6, L)
    sd = mr.sequential(450, 128, 6, L).state_dict()
    keys = list(sd.keys())
    assert keys == [f"{2 * i}.{n}" for i in range(L) for n in ("weight", "bias")]
    off = 0
    for i in range(L):
        assert info.off_w[i] == off; off += sd[f"{2 * i}.weight"].numel()
        assert info.off_b[i] == off; off += sd[f"{2 * i}.bias"].numel()
    assert info.n_flat == off and info.rows_per_tile == 32 and info.n_launches_step == 5
    m = models.MLP(450, 128, 6, L)
    assert list(m.state_dict().keys()) == keys and [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in sd.values()]
    assert list(m._spec.param_offsets().values()) == [(int(info.off_w[i // 2]) if i % 2 == 0 else int(info.off_b[i // 2]), v.numel()) for i, v in enumerate(sd.values())]
    macs = sum(v.numel() for k, v in sd.items() if k.endswith("weight"))
    assert info.flops_fwd == 2 * macs and info.flops_bwd == 4 * macs - 2 * 128 * 450


def test_same_seed_same_initial_weights_as_the_reference_module():
    torch.manual_seed(12); m = models.MLP(30, 128, 4, 4)
    torch.manual_seed(12); r = mr.sequential(30, 128, 4, 4)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), r.state_dict().values()))
    assert isinstance(m[1], nn.ReLU) and isinstance(m[0], nn.Linear) and len(m) == 7


@pytest.mark.parametrize("args,text", [((450, 64, 4, 3), "hidden must be 128, 256, 384 or 512"), ((450, 640, 4, 3), "hidden must be 128, 256, 384 or 512"),
                                       ((0, 128, 4, 3), "in_channels must be in 1..16384"), ((16385, 128, 4, 3), "in_channels must be in 1..16384"),
                                       ((450, 128, 17, 3), "out_channels must be in 1..16"), ((450, 128, 4, 1), "num_layers must be in 2..16"),
                                       ((450, 128, 4, 17), "num_layers must be in 2..16")])
def test_compile_host_refusals_name_the_limit(args, text):
    with pytest.raises(engine.MshgnnError, match=text.replace(".", r"\.")) as ex:
        engine.mlp_compile_host(*args)
    assert "(-2)" in str(ex.value)      # MSHGNN_EUNSUPPORTED
    assert not engine.mlp_supported(*args)


def test_compile_host_refuses_odd_out_with_cross_entropy_and_takes_the_limits():
    with pytest.raises(engine.MshgnnError, match="even out_channels"):
        engine.mlp_compile_host(450, 128, 3, 3, loss="ce")
    engine.mlp_compile_host(450, 128, 3, 3, loss="mse")
    for args in ((1, 128, 1, 2), (16384, 512, 16, 16), (8100, 384, 8, 8)):
        assert engine.mlp_compile_host(*args).n_flat > 0 and engine.mlp_supported(*args)
    with pytest.raises(engine.MshgnnError, match="bf16"):
        engine.mlp_compile_host(450, 128, 4, 3, dtype="f32")


def test_struct_sizes_of_the_new_structs():
    import ctypes as C
    lib = engine.load_library()
    assert lib.mshgnn_struct_size(5) == C.sizeof(engine.MshgnnMlpDesc) and lib.mshgnn_struct_size(6) == C.sizeof(engine.MshgnnMlpInfo)
    assert lib.mshgnn_struct_size(7) == C.sizeof(engine.MshgnnMlpInput) and lib.mshgnn_struct_size(99) == 0 and lib.mshgnn_abi_version() == 6
    for name in ("mshgnn_mlp_forward", "mshgnn_mlp_backward", "mshgnn_mlp_step"):
        assert name in engine.EXPORTS
    assert lib.mshgnn_mlp_forward(None, None, None, None, None, 1, 0, None) == -1 and b"mshgnn_mlp_forward" in lib.mshgnn_last_error()
    assert lib.mshgnn_mlp_step(None, None, 0, None, None, None, None, None, None, 1, None) == -1 and b"mshgnn_mlp_step" in lib.mshgnn_last_error()


def test_wrapper_constructors_and_attribute_names():
    ref_mlp = ["in_channels", "hidden_channels", "out_channels", "num_layers", "batch_size", "optimizer", "lr", "regression", "activation_fn"]
    assert list(inspect.signature(wrappers.MLP_Lightning.__init__).parameters)[1:] == ref_mlp
    assert list(inspect.signature(wrappers.COM_MLP_Lightning.__init__).parameters)[1:len(ref_mlp) + 2] == ref_mlp + ["data_path"]
    assert inspect.signature(wrappers.MLP_Lightning.__init__).parameters["lr"].default == 0.003
    w = wrappers.MLP_Lightning(40, 128, 8, 3, 32, regression=False)
    assert isinstance(w.mlp_model, models.MLP) and w.model is w.mlp_model and w.batch_size == 32 and w.regression is False
    assert list(w.state_dict().keys()) == [f"mlp_model.{2 * i}.{n}" for i in range(3) for n in ("weight", "bias")]
    c = wrappers.COM_MLP_Lightning(24, 128, 6, 3, 32, stats=(np.zeros(6), np.ones(6)))
    assert c.model.num_bases == 1 and c.model.num_dimensions_per_base == 6
    assert list(c.state_dict().keys()) == [f"model.{2 * i}.{n}" for i in range(3) for n in ("weight", "bias")]
    with pytest.raises(ValueError, match="2 or greater"):
        wrappers.MLP_Lightning(40, 128, 8, 1, 32)
    for wr in (w, c):
        assert type(wr.configure_optimizers()).__name__ == "FlatAdam" and callable(wr.step_helper_function)


@pytest.mark.parametrize("model_type", ["mlp", "mlp_com"])
def test_checkpoint_round_trip(model_type, tmp_path):
    torch.manual_seed(2)
    m = models.MLP(40, 128, 6, 4)
    ck = checkpoint.mlp_to_lightning_checkpoint(m, model_type)
    prefix = "mlp_model." if model_type == "mlp" else "model."
    assert list(ck["state_dict"].keys()) == [prefix + k for k in m.state_dict().keys()]
    path = os.path.join(tmp_path, "mlp.ckpt")
    torch.save(ck, path)
    back = checkpoint.mlp_from_checkpoint(path, model_type)
    assert (back.in_channels, back.hidden_channels, back.out_channels, back.num_layers) == (40, 128, 6, 4)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), back.state_dict().values()))
    # the reference's wrapper would load these keys by name
    wr = wrappers.MLP_Lightning(40, 128, 6, 4, 8) if model_type == "mlp" else wrappers.COM_MLP_Lightning(40, 128, 6, 4, 8, stats=(np.zeros(6), np.ones(6)))
    wr.load_state_dict(ck["state_dict"], strict=True)
    with pytest.raises(ValueError, match="weights say"):
        checkpoint.mlp_from_checkpoint(ck, model_type, hidden_channels=256)


def test_mlp_engine_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.MLPEngine(450, 128, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        models.MLP(450, 128, 4, 3)(torch.zeros(2, 450))
