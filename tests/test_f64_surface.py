"""The "f64" precision and the operators' compute dtype, as far as they show without a GPU: names accepted and refused, parameters made fp64 (by
set_precision and by MSHGNN_DTYPE=f64 at construction) and fp32 again, every one-call / series route stepping aside, the exports declared."""
import pytest
import torch

from morphsym_hgnn_amd import engine as eng
from morphsym_hgnn_amd import models, ops
from tests import helpers
from tests.test_models import _build


def test_compute_dtype_names_and_scope():
    assert ops.get_compute_dtype() == "f32"
    with ops.compute_dtype("f64"):
        assert ops.get_compute_dtype() == "f64"
        with ops.compute_dtype("f32"):
            assert ops.get_compute_dtype() == "f32"
        assert ops.get_compute_dtype() == "f64"
    assert ops.get_compute_dtype() == "f32"
    with pytest.raises(RuntimeError, match="boom"):      # restored on the way out of a failing block too
        with ops.compute_dtype("f64"):
            raise RuntimeError("boom")
    assert ops.get_compute_dtype() == "f32"
    assert ops.set_compute_dtype("f64") == "f32" and ops.set_compute_dtype("f32") == "f64"
    for bad in ("bf16", "x3", "float64", ""):
        with pytest.raises(ValueError):
            ops.set_compute_dtype(bad)
    assert ops.get_compute_dtype() == "f32"
    with ops.compute_dtype("f64"), pytest.raises(RuntimeError, match="no CPU fallback"):      # the mode adds no CPU path
        ops.linear(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.float64))


def test_exports_are_listed():
    names = ["mshgnn_op_gemm_f64", "mshgnn_op_gemm_f64_workspace", "mshgnn_op_aggregate_f64", "mshgnn_op_colsum_f64", "mshgnn_op_colsum_f64_workspace"]
    assert all(n in eng.EXPORTS for n in names) and eng.ABI_VERSION == 6      # no struct changed: the ABI version stays


@pytest.mark.parametrize("name", ["a1c2_h128_L3_d3_B3", "solok4com_h128_L3_B5", "mi_h128_L2_d3_B2"])
def test_set_precision_f64_makes_the_parameters_fp64_and_back(name):
    torch.set_default_dtype(torch.float32)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case(name)
    m = _build(case, spec)
    for t in spec.node_types:
        m.encoder.lins[t].materialize(spec.widths[t])
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    assert m.set_precision("f64") is m and m._precision == "f64" and not m._fused_ok()
    assert all(p.dtype == torch.float64 and torch.equal(p, before[k].double()) for k, p in m.named_parameters())
    src = {k: v.double() * (1.0 + 2.0 ** -40) for k, v in params.items()}
    m.load_state_dict(src)
    assert all(torch.equal(p.detach(), src[k]) for k, p in m.named_parameters())      # a reference checkpoint keeps every bit
    m.set_precision("f64")                                                          # (again: nothing changes)
    assert all(torch.equal(p.detach(), src[k]) for k, p in m.named_parameters())
    m.set_precision("x3")
    assert m._fused_ok() and all(p.dtype == torch.float32 and torch.equal(p.detach(), src[k].float()) for k, p in m.named_parameters())
    m.set_precision("bf16")      # between the engine plans nothing is converted
    assert all(p.dtype == torch.float32 for p in m.parameters())
    with pytest.raises(ValueError, match="'f64'"):
        m.set_precision("f16")


def test_precision_from_the_environment(monkeypatch):
    monkeypatch.setenv("MSHGNN_DTYPE", "f64")
    torch.set_default_dtype(torch.float32)
    case, spec, fx, x_dict, y, params, ei = helpers.load_case("a1c2_h128_L3_d3_B3")
    m = _build(case, spec)
    assert m._precision == "f64" and m.decoder.weight.dtype == torch.float64 and m.base_transform[0].weight.dtype == torch.float64
    assert all(p.dtype == torch.float64 for k, p in m.named_parameters() if not k.startswith("encoder."))      # (the lazy encoder follows at its first forward)
    mlp = models.MLP(30, 128, 6, 3)
    assert mlp._precision == "f64" and all(p.dtype == torch.float64 for p in mlp.parameters()) and not mlp._fused()
    monkeypatch.setenv("MSHGNN_DTYPE", "x3")
    assert all(p.dtype == torch.float32 for p in models.MLP(30, 128, 6, 3).parameters())
