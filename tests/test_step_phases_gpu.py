"""The decoder + loss tail of the compile-time programs is compiled for the program's output channels and output nodes and, in the whole-tile kernels, without
the row predicate (csrc/mshgnn_device.hpp, DecFacts): vector moves of a node's labels and outputs off uniform bases, row / half swaps instead of shuffles for the
wave's four rows, the same additions in the same order.  The interpreting kernels keep the run-time tail, so they are the yardstick: for every built-in program
-- MiniCheetah-K4 with the cross-entropy tail and aliased stashes, the Solo COM programs with the output type first, six channels and (S4) a single output node
-- the one-call step must give the interpreter's bits in the output, the loss, the whole flat gradient and every dX stash, at one whole tile (16 windows), a
whole tile plus a one-window tile (17: the predicated form) and three tiles (48).  The split plan's kernels keep the run-time tail; two of its programs ride along."""
import pytest
import torch

import bench
from morphsym_hgnn_amd import engine as eng, synth

pytestmark = pytest.mark.gpu
CASES = [("bf16", "a1c2", 3, "A1C2_L3"), ("bf16", "a1c2", 8, "A1C2_L8"), ("bf16", "mck4", 8, "MCK4_L8"), ("bf16", "mcc2", 8, "MCC2_L8"),
         ("bf16", "solo", 8, "SOLO_L8"), ("bf16", "solo_s4", 8, "SOLO_S4_L8"), ("bf16", "mi_quad", 8, "MI_QUAD_L8"),
         ("x3", "a1c2", 3, "X3_A1C2_L3"), ("x3", "mck4", 8, "X3_MCK4_L8")]
BATCHES = (16, 17, 48)


def _target(e, spec, y, B):
    if spec.regression:
        return y.to(e.device, torch.float32).reshape(-1).contiguous()
    return y.to(e.device, torch.int32).reshape(B, -1).contiguous()


def _stashes(e, spec, B):
    return [e.grad_hidden(B, l).clone() for l in range(spec.num_layers + 1)]


def _one_call(e, spec, x, y, flat, B):
    """(out, loss, flat gradient, dX_0 .. dX_L) of the one-call step; the workspace starts from zeros, so rows no kernel writes compare equal too"""
    e.workspace(B, True).zero_()
    xs = e.cast_inputs(x)
    t = _target(e, spec, y, B)
    out, loss, g = (e.step_mse if spec.regression else e.step_ce)(xs, flat, t, B)
    torch.cuda.synchronize()
    return [out.clone(), loss.clone(), g.clone()] + _stashes(e, spec, B)


def _two_call(e, spec, x, y, flat, B):
    e.workspace(B, True).zero_()
    xs = e.cast_inputs(x)
    t = _target(e, spec, y, B)
    out = e.forward(xs, flat, B, training=True).clone()
    loss, g = (e.backward_mse if spec.regression else e.backward_ce)(xs, flat, out, t, B)
    torch.cuda.synchronize()
    return [out, loss.clone(), g.clone()] + _stashes(e, spec, B)


def _names(spec):
    return ["out", "loss", "grad"] + [f"dX_{l}" for l in range(spec.num_layers + 1)]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.element_size() == 4 else a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int32) if b.element_size() == 4 else b.contiguous().view(torch.int16))


def _engines(monkeypatch, spec, plan, name):
    monkeypatch.setenv("MSHGNN_SLAB", "2")          # the slab kernels also below one tile per CU
    monkeypatch.setenv("MSHGNN_SPEC", "1")
    e1 = eng.Engine(spec, plan)
    monkeypatch.setenv("MSHGNN_SPEC", "0")
    e0 = eng.Engine(spec, plan)
    assert e1.specialised == name and e0.specialised == "", (e1.specialised, e0.specialised)
    return e1, e0


def _check_step(e1, e0, spec, x, y, flat, B, tag):
    r1 = _one_call(e1, spec, x, y, flat, B)
    r0 = _one_call(e0, spec, x, y, flat, B)
    for what, a, b in zip(_names(spec), r1, r0):
        assert _same_bits(a, b), f"{tag} B={B}: {what} differs from the interpreter, max abs {float((a.float() - b.float()).abs().max())}"
    assert float(r1[2].abs().max()) > 0 and torch.isfinite(r1[1]).all() and float(r1[3].abs().max()) > 0
    again = _one_call(e1, spec, x, y, flat, B)
    for what, a, b in zip(_names(spec), r1, again):
        assert _same_bits(a, b), f"{tag} B={B}: {what} differs between two runs"
    return r1


def _check_two_call(e1, spec, x, y, flat, B, tag, r1):
    """forward + backward_mse / backward_ce against the one-call step of the same engine, held to the project's contract for this pair
    (tests/test_engine_gpu.py::test_one_call_step_equals_forward_plus_backward): the same output bits; the decoder backward of the two-call route is its own
    launch, which sums the loss and the decoder's gradients in another order (loss within 1e-5, decoder gradients within 2e-5 of their largest entry, as
    there).  Every other launch of the backward sweep sees the same dX_L bits, so the stashes and every other gradient are the same bits."""
    r2 = _two_call(e1, spec, x, y, flat, B)
    names = _names(spec)
    assert _same_bits(r1[0], r2[0]), f"{tag} B={B}: two-call output differs"
    for what, a, b in list(zip(names, r1, r2))[3:]:
        assert _same_bits(a, b), f"{tag} B={B}: two-call {what} differs, max abs {float((a.float() - b.float()).abs().max())}"
    assert abs(float(r1[1]) - float(r2[1])) <= 1e-5 * abs(float(r1[1])), (tag, B, float(r1[1]), float(r2[1]))
    ga, gb = eng.unflatten(spec, r1[2]), eng.unflatten(spec, r2[2])
    for k in ga:
        if k.startswith("decoder"):
            assert float((ga[k] - gb[k]).abs().max()) <= 2e-5 * float(ga[k].abs().max()), (tag, B, k)
        else:
            assert _same_bits(ga[k], gb[k]), f"{tag} B={B}: two-call gradient {k} differs, max abs {float((ga[k] - gb[k]).abs().max())}"


@pytest.mark.parametrize("plan,config,layers,name", CASES)
def test_program_step_is_the_interpreters_bits(monkeypatch, plan, config, layers, name):
    spec = bench.build_spec(layers, config)
    e1, e0 = _engines(monkeypatch, spec, plan, name)
    flat = eng.flatten_params(spec, synth.make_params(13, spec.param_shapes()), e1.device)
    for B in BATCHES:
        x, y = bench.make_batch(spec, B, 71 + B)
        r1 = _check_step(e1, e0, spec, x, y, flat, B, name)
        _check_two_call(e1, spec, x, y, flat, B, name, r1)


def test_output_mask_with_zeros_is_refused_and_other_signs_run(monkeypatch):
    """The plan accepts +-1 output masks only (mshgnn_plan_create: "output mask must be +1 or -1"), so a mask with zeros never reaches a kernel: that refusal is
    pinned here, and the tail's mask operand is exercised with the signs of two of the twelve entries flipped instead."""
    spec = bench.build_spec(3, "a1c2")
    zeros = spec.output_mask().clone()
    zeros[0, 1] = 0.0; zeros[3, 2] = 0.0
    spec.output_mask = lambda: zeros
    with pytest.raises(eng.MshgnnError, match="output mask"):
        eng.Engine(spec, "bf16")
    spec = bench.build_spec(3, "a1c2")
    mask = spec.output_mask().clone()
    mask[0, 1] = -mask[0, 1]; mask[3, 2] = -mask[3, 2]
    spec.output_mask = lambda: mask
    e1, e0 = _engines(monkeypatch, spec, "bf16", "A1C2_L3")
    flat = eng.flatten_params(spec, synth.make_params(17, spec.param_shapes()), e1.device)
    ref = bench.build_spec(3, "a1c2")
    monkeypatch.setenv("MSHGNN_SPEC", "1")
    er = eng.Engine(ref, "bf16")
    for B in (16, 17):
        x, y = bench.make_batch(spec, B, 91 + B)
        r1 = _check_step(e1, e0, spec, x, y, flat, B, "A1C2_L3 flipped mask")
        out, out_ref = r1[0].reshape(B, 4, 3), _one_call(er, ref, x, y, flat, B)[0].reshape(B, 4, 3)
        assert torch.equal(out[:, 0, 1], -out_ref[:, 0, 1]) and torch.equal(out[:, 3, 2], -out_ref[:, 3, 2]) and torch.equal(out[:, 1], out_ref[:, 1])
        _check_two_call(e1, spec, x, y, flat, B, "A1C2_L3 flipped mask", r1)


@pytest.mark.parametrize("config,layers,name", [("a1c2", 3, "A1C2_L3"), ("mck4", 8, "MCK4_L8")])
def test_labels_all_equal(monkeypatch, config, layers, name):
    """Every label the same value (regression: one constant, classification: every foot in contact)."""
    spec = bench.build_spec(layers, config)
    e1, e0 = _engines(monkeypatch, spec, "bf16", name)
    flat = eng.flatten_params(spec, synth.make_params(19, spec.param_shapes()), e1.device)
    for B in (16, 17):
        x, y = bench.make_batch(spec, B, 101 + B)
        y = torch.full_like(y, 0.25) if spec.regression else torch.ones_like(y)
        r1 = _check_step(e1, e0, spec, x, y, flat, B, name + " equal labels")
        _check_two_call(e1, spec, x, y, flat, B, name + " equal labels", r1)


def test_program_of_other_output_channels_is_refused(monkeypatch):
    """The A1-C2 topology at 3 layers as a CLASSIFICATION model (two logits per foot): its slab tables are the ints of the A1C2_L3 program, whose tail is compiled
    for three output channels -- spec_matches must refuse it (the interpreter runs: speed, never results)."""
    import yaml, os
    from morphsym_hgnn_amd import topology
    from morphsym_hgnn_amd.spec import ModelSpec
    with open(os.path.join(bench.ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")) as f:
        group = yaml.safe_load(f)
    spec = ModelSpec(kind="c2", topology=topology.a1_c2(), hidden=128, num_layers=3, widths=synth.feature_widths("c2", False), regression=False,
                     grf_dimension=3, group=group)
    assert spec.out_channels == 2
    monkeypatch.setenv("MSHGNN_SLAB", "2"); monkeypatch.setenv("MSHGNN_SPEC", "1")
    e1 = eng.Engine(spec, "bf16")
    monkeypatch.setenv("MSHGNN_SPEC", "0")
    e0 = eng.Engine(spec, "bf16")
    assert e1.specialised == "" and e0.specialised == ""
    flat = eng.flatten_params(spec, synth.make_params(23, spec.param_shapes()), e1.device)
    for B in (16, 17):
        x, y = bench.make_batch(spec, B, 111 + B)
        r1, r0 = _one_call(e1, spec, x, y, flat, B), _one_call(e0, spec, x, y, flat, B)
        for what, a, b in zip(_names(spec), r1, r0):
            assert _same_bits(a, b), f"B={B}: {what} differs"
        assert float(r1[2].abs().max()) > 0 and torch.isfinite(r1[1]).all()
