"""sha1 of the flat gradient (and loss bits) of one seeded step per configuration: run under two builds of the library (MSHGNN_LIB) to compare them bit for bit.
  hgnn  one step per HGNN configuration
  mlp   the MLP baselines (csrc/mshgnn_mlp.hip) on data that rounds: tests/mlp_reference.random_case on the rows of its EXACT_MATRIX, one batch each; both dtypes,
        both losses; the step, forward + backward and the inference forward; on bf16 also the series step.  Per line the sha1 of out, the loss bits, the flat
        gradient and the raw bytes of the layer-1 stash.
usage: python tools/grad_hash.py [hgnn] [mlp]      (nothing named: both)"""
import hashlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from morphsym_hgnn_amd import engine as eng, synth


def sha(t):
    return hashlib.sha1(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def hgnn():
    for config, L, dtype, B in (("a1c2", 3, "bf16", 8192), ("a1c2", 3, "bf16", 48), ("a1c2", 3, "bf16", 50), ("a1c2", 3, "x3", 1040), ("a1c2", 3, "f32", 64), ("mck4", 8, "bf16", 4096), ("solo", 8, "bf16", 8192)):
        spec = bench.build_spec(L, config)
        e = eng.Engine(spec, dtype)
        flat = eng.flatten_params(spec, synth.make_params(3, spec.param_shapes()), e.device)
        x, y = bench.make_batch(spec, B, 17)
        xs = e.cast_inputs(x)
        if spec.regression:
            out, loss, g = e.step_mse(xs, flat, y.to(e.device, torch.float32).reshape(-1), B)
        else:
            out, loss, g = e.step_ce(xs, flat, y.to(e.device, torch.int32).reshape(B, -1).contiguous(), B)
        torch.cuda.synchronize()
        print(config, L, dtype, B, "loss", float(loss), "grad sha1", hashlib.sha1(g.cpu().numpy().tobytes()).hexdigest()[:16], "nonzero", int((g != 0).sum()))


MLP_BATCH = (17, 1000, 8193, 17, 1000, 17, 17)      # one batch of each row of EXACT_MATRIX


def mlp():
    from torch import nn
    from tests import mlp_reference as mr
    dev = "cuda:0"

    def stash1(e, B):      # the layer-1 stash as stored: bf16 [B][H], split plan [B][hi H | lo H]
        off = int(e.lib.mshgnn_mlp_stash_offset(e._plan, B, 1))
        return e.workspace(B, True)[off:off + B * e.hidden * (4 if e.dtype == "x3" else 2)]

    for (in_channels, T, hidden, L, out_channels, _), B in zip(mr.EXACT_MATRIX, MLP_BATCH):
        c = mr.random_case(in_channels, hidden, out_channels, L, B, seed=in_channels + L)
        flat = mr.flatten(c["params"]).float().to(dev)
        y, labels = c["y"].float().to(dev).contiguous(), c["labels"].to(dev).contiguous()
        gout = torch.randn(B, out_channels, generator=torch.Generator().manual_seed(B)).to(dev)
        for dtype in ("bf16", "x3"):
            e = eng.MLPEngine(in_channels, hidden, out_channels, L, dtype, dev)
            # the split plan's rows are fp32: scaled by 1 + 3 / 1024, so that their lo halves are not zero
            x = e.cast_input(c["x"] if dtype == "bf16" else c["x"] * (1 + 3 / 1024))
            tag = f"mlp in {in_channels} H {hidden} L {L} out {out_channels} B {B} {dtype}"
            for loss in ("mse", "ce"):
                out, lv, g = e.step_mse(x, flat, y) if loss == "mse" else e.step_ce(x, flat, labels)
                torch.cuda.synchronize()
                print(tag, "step", loss, "out", sha(out), "loss", sha(lv), "grad", sha(g), "stash1", sha(stash1(e, B)))
            out = e.forward(x, flat, training=True)
            g = e.backward(x, flat, gout)
            torch.cuda.synchronize()
            print(tag, "forward+backward", "out", sha(out), "grad", sha(g), "stash1", sha(stash1(e, B)))
            print(tag, "inference", "out", sha(e.forward(x, flat, training=False)))
    # the series step (bf16): the store of tests/test_mlp_gpu.py::test_series_methods_equal_assemble_then_dense; history 7 gathers element by element
    from morphsym_hgnn_amd import windows
    from tests import test_window_symmetry as ws
    for T in (20, 7):
        store = windows.SequenceStore(ws.SEQ4, windows.minicheetah_mlp_recipe(ws.JP, ws.FP, T, False), dtype="bf16", device=dev)
        e = eng.MLPEngine(T * 54, 128, 8, 3, "bf16", dev)
        assert e._series_ok(store)
        torch.manual_seed(3)
        flat = mr.flatten([(m.weight.detach(), m.bias.detach()) for m in mr.sequential(T * 54, 128, 8, 3) if isinstance(m, nn.Linear)]).float().to(dev)
        n = len(store)
        starts = torch.randint(0, n, (77,), generator=torch.Generator().manual_seed(2))
        starts[0], starts[-1] = 0, n - 1
        starts = starts.to(dev)
        for loss, step in (("ce", e.step_ce_series), ("mse", e.step_mse_series)):
            targets = None if loss == "ce" else torch.randn(77, 8, generator=torch.Generator().manual_seed(5)).to(dev)      # (the recipe's labels are the 4 contact flags)
            t, out, lv, g = step(store, starts, flat, targets=targets)
            torch.cuda.synchronize()
            print(f"mlp series T {T} in {T * 54} B 77 bf16 step", loss, "targets", sha(t), "out", sha(out), "loss", sha(lv), "grad", sha(g), "stash1", sha(stash1(e, 77)))


if __name__ == "__main__":
    what = sys.argv[1:] or ["hgnn", "mlp"]
    if "hgnn" in what:
        hgnn()
    if "mlp" in what:
        mlp()
