"""Whole-sequence GRU / SimpleRnn HIP kernels (csrc/gru.hip) and the layers on top of them, against the per-step
equations evaluated in fp64 on the CPU from the same (already rounded, for 16-bit) inputs and weights."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.ops import fallback, rnn_native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# fp32 / bf16: the bounds of tests/test_gpu_lstm.py. fp16: twice the error of the fp16 LSTM kernels (out, hT, cT, dh0,
# dc0 of lstm_seq_fwd / lstm_seq_bwd at H 32 / 64 / 256, mb 37, T 11) under the same measure on MI355X, FP16_LSTM_ERR.
FP16_LSTM_ERR = 1.37e-3
TOL = {torch.float32: 2e-4, torch.bfloat16: 4e-2, torch.float16: 2 * FP16_LSTM_ERR}
T = 7


def _close(a, b, tol, what):
    """The measure of tests/test_gpu_lstm.py: max abs error over max(1, max |reference|)."""
    a, b = a.double().cpu(), b.double().cpu()
    err, scale = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
    print(f"{what}: err/scale {err / scale:.3e} (bound {tol:.1e})")
    assert err <= tol * scale, f"{what}: max abs err {err} (scale {scale})"


def _reference(cell, zx, RW, bRn, h0, mask, eps, t_end, pos=None):
    """fp64 per-step equations. Returns out [T, mb, H], hT, dz ([T, mb, 4H] = [dzr | dzz | dzn | dzn*r] for the GRU,
    [T, mb, H] for the RNN cells), dh0. ``pos``: where relu' is 1 (default: where the reference's own output is > 0)."""
    H = RW.shape[0]
    h, outs, cache = h0, [], []
    for t in range(T):
        a = h @ RW
        if cell == "gru":
            r, z = torch.sigmoid(zx[t, :, :H] + a[:, :H]), torch.sigmoid(zx[t, :, H:2 * H] + a[:, H:2 * H])
            q = a[:, 2 * H:] + bRn
            n = torch.tanh(zx[t, :, 2 * H:] + r * q)
            cache.append((r, z, n, q, h))
            hn = (1 - z) * n + z * h
        else:
            hn = torch.tanh(zx[t] + a) if cell == "tanh" else torch.relu(zx[t] + a)
        h = hn * mask[:, t:t + 1]
        outs.append(h)
    dz = torch.zeros(T, zx.shape[1], (4 if cell == "gru" else 1) * H, dtype=torch.float64)
    dh_next = torch.zeros_like(h0)
    for t in range(T - 1, t_end - 1, -1):
        dh = (eps[t] + dh_next) * mask[:, t:t + 1]
        if cell == "gru":
            r, z, n, q, hp = cache[t]
            dzn = dh * (1 - z) * (1 - n * n)
            dzz, dzr = dh * (hp - n) * z * (1 - z), dzn * q * r * (1 - r)
            dz[t] = torch.cat([dzr, dzz, dzn, dzn * r], 1)
            dh_next = dh * z + torch.cat([dzr, dzz, dzn * r], 1) @ RW.t()
        else:
            dz[t] = dh * (1 - outs[t] ** 2) if cell == "tanh" else dh * (outs[t] > 0 if pos is None else pos[t])
            dh_next = dz[t] @ RW.t()
    return torch.stack(outs), h, dz, dh_next


# H per kernel instance (csrc/gru.hip pick_nt): 32 -> NT 1, 48 -> NT 1 with H % 32 != 0 (fp32 only), 160 -> NT 2,
# 320 -> NT 4; 40 is refused
@pytest.mark.parametrize("mb,t_end", [(5, 0), (37, 3), (37, 0)])
@pytest.mark.parametrize("H", [32, 48, 160, 320, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("cell", ["gru", "tanh", "relu"])
def test_sequence_kernels_match_fp64_equations(cell, dtype, H, mb, t_end):
    g = torch.Generator().manual_seed(H + mb)
    G = 3 if cell == "gru" else 1
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    zx, RW = (rnd(T, mb, G * H) * 0.7).to(dtype), (rnd(H, G * H) * (1.2 / H ** 0.5)).to(dtype)
    bRn, h0, eps = rnd(H) * 0.3, rnd(mb, H) * 0.5, rnd(T, mb, H)
    mask = torch.ones(mb, T, dtype=torch.float64)
    mask[1, 3:5] = 0                                            # zeros in the middle of a row
    mask[mb - 1, 4:] = 0                                        # ... and at the end of one
    mask[2, T - 1] = 0
    f32 = lambda t: t.float().to(DEV)  # noqa: E731
    zd, RWd = zx.to(DEV), RW.to(DEV)
    if cell == "gru":
        fwd = rnn_native.gru_seq_fwd(zd, RWd, f32(bRn), H, f32(h0), f32(mask), True)
    else:
        fwd = rnn_native.rnn_seq_fwd(zd, RWd, H, cell, f32(h0), f32(mask))
    if H == 40 or (H == 48 and dtype != torch.float32):
        assert fwd is None
        return
    out = fwd[0]
    # relu' jumps at 0: a pre-activation within rounding of 0 may land on either side, which the check of ``out``
    # bounds; the backward reference then takes the side the forward took
    want = _reference(cell, zx.double(), RW.double(), bRn, h0, mask, eps, t_end, pos=(out > 0).cpu())
    if cell == "gru":
        _, hT, gates, _ = fwd
        dz, dh0 = rnn_native.gru_seq_bwd(f32(eps), gates, out, f32(h0), RWd, H, f32(mask), None, t_end)
    else:
        hT = fwd[1]
        dz, dh0 = rnn_native.rnn_seq_bwd(f32(eps), out, RWd, H, cell, f32(mask), None, t_end)
    for name, got, ref in zip(("out", "hT", "dz", "dh0"), (out, hT, dz, dh0), want):
        _close(got, ref, TOL[dtype], name)


def _pair(layer, nIn=12, H=32):
    """The same GRU / SimpleRnn -> RnnOutputLayer network on the GPU in fp32 and on the CPU in fp64, equal parameters."""
    nets = []
    for dev, dt in ((DEV, DataType.FLOAT), (torch.device("cpu"), DataType.DOUBLE)):
        conf = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(Sgd(0.5)).list()
                .layer(0, layer.Builder().nIn(nIn).nOut(H).activation(Activation.TANH).build())
                .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).nOut(4).activation(Activation.SOFTMAX).build())
                .setInputType(InputType.recurrent(nIn)).build())
        net = MultiLayerNetwork(conf)
        net.init(device=dev)
        nets.append(net)
    p = torch.randn(nets[1].numParams(), generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 0.3
    nets[0].setParams(p.float().to(DEV))
    nets[1].setParams(p.clone())
    return nets, p


def _batch(nIn=12, mb=5, Tn=T):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(mb, nIn, Tn, generator=g, dtype=torch.float64)
    y = torch.nn.functional.one_hot(torch.randint(0, 4, (mb, Tn), generator=g), 4).permute(0, 2, 1).double()
    return x, y


@pytest.mark.parametrize("layer", [GRU, SimpleRnn], ids=["gru", "simple_rnn"])
def test_fit_step_matches_cpu_fp64(layer):
    """One SGD step: score and applied update (= learning rate x flat gradient) of the GPU fp32 network against the
    CPU fp64 one, with no helper fallback."""
    (gpu, cpu), p0 = _pair(layer)
    x, y = _batch()
    fallback.reset()
    gpu.fit(x.float().to(DEV), y.float().to(DEV))
    cpu.fit(x, y)
    assert gpu.helperCountFail() == 0, fallback.summary()
    assert abs(gpu.score() - cpu.score()) <= 1e-3 * abs(cpu.score())
    ug, uc = p0 - gpu.params().double().cpu(), p0 - cpu.params()
    assert uc.norm() > 0
    rel = ((ug - uc).norm() / uc.norm()).item()
    print(f"{layer.__name__}: update rel err {rel:.3e}")
    assert rel <= 1e-3


def test_gru_time_steps_reproduce_activate():
    (gpu, _), _ = _pair(GRU)
    x = _batch()[0].float().to(DEV)
    whole = gpu.output(x)
    steps = torch.stack([gpu.rnnTimeStep(x[:, :, t]) for t in range(T)], dim=2)
    _close(steps, whole, TOL[torch.float32], "rnnTimeStep")


def test_simple_rnn_recurrence_launches_no_per_step_matmul():
    """The launch list of a SimpleRnn fit step (torch.profiler, as tests/test_gpu_step_kernels.py lists it): one
    forward and one backward sequence kernel, and a GEMM count that does not grow with the sequence length."""
    from torch.profiler import ProfilerActivity, profile
    (gpu, _), _ = _pair(SimpleRnn)
    counts = []
    for Tn in (T, 2 * T):
        x, y = (t.float().to(DEV) for t in _batch(Tn=Tn))
        gpu.fit(x, y)                                           # warm-up: kernel choice per shape
        gpu.fit(x, y)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gpu.fit(x, y)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        assert sum("gru_fwd_kernel" in n for n in names) == 1 and sum("gru_bwd_kernel" in n for n in names) == 1, names
        counts.append(sum("gemm" in n and "reduce" not in n for n in names))
    assert counts[0] == counts[1] > 0, counts
