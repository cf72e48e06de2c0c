"""The fp8 key/value cache off the GPU: the row format of csrc/attention_decode.hip as the torch reference functions of
ops/transformer_native.py write it (against a direct computation), the ``cacheDataType`` configuration field, and an
fp32 CPU network decoding with the fp8 cache (against an explicit emulation on its stored state)."""
import json

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.ops import transformer_native as TN

CPU = torch.device("cpu")


def _groups(dt, H, D):
    """[2, 6, 2E] in dt: randn * 0.8 with an all-zero group, one scaled by 2^-10 and one by 2^6."""
    g = torch.Generator().manual_seed(17 + H + D)
    x = torch.randn(2, 6, 2 * H * D, generator=g) * 0.8
    x[0, 0, :D] = 0.0
    x[0, 1, D:2 * D] *= 2.0 ** -10
    x[1, 2, -D:] *= 2.0 ** 6
    return x.to(dt)


def _direct(x, H, D):
    """codes [.., 2H, D] (uint8), ex [.., 2H] straight from the format's definition."""
    g = x.float().reshape(*x.shape[:-1], 2 * H, D)
    amax = g.abs().amax(-1)
    m, e = torch.frexp(amax)
    ex = torch.where(m <= 0.875, e - 9, e - 8)
    ex = torch.where(amax == 0, torch.zeros_like(ex), ex).clamp(-126, 127)
    codes = torch.ldexp(g, -ex.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return codes, ex


@pytest.mark.parametrize("H,D", [(2, 64), (3, 128), (12, 64)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_quantize_reference_is_the_format(dt, H, D):
    x = _groups(dt, H, D)
    E2, R = 2 * H * D, TN.kv_fp8_row_bytes(H, D)
    q = TN.kv_fp8_quantize_reference(x, H)
    assert q.dtype == torch.uint8 and q.shape == (2, 6, R)
    codes, ex = _direct(x, H, D)
    assert torch.equal(q[..., :E2], codes.view(torch.uint8).reshape(2, 6, E2))
    assert torch.equal(q[..., E2:E2 + 2 * H], (ex + 127).to(torch.uint8))
    assert torch.count_nonzero(q[..., E2 + 2 * H:]) == 0
    assert q[0, 0, E2] == 127 and torch.count_nonzero(q[0, 0, :D]) == 0          # the all-zero group: ex = 0
    top = codes.float().abs().amax(-1)
    nz = x.float().reshape(2, 6, 2 * H, D).abs().amax(-1) > 0
    assert (~nz).sum() == 1
    assert ((top >= 224) & (top <= 448))[nz].all(), "the largest code of a non-zero group lies in [224, 448]"
    d32 = TN.kv_fp8_dequantize_reference(q, H, D, torch.float32)
    assert torch.equal(d32, torch.ldexp(codes.float(), ex.unsqueeze(-1)).reshape(2, 6, E2))
    if dt != torch.float32:                                  # 16-bit inputs: the values are exact in their dtype
        assert torch.equal(TN.kv_fp8_dequantize_reference(q, H, D, dt).float(), d32)
    # a code has 4 significant bits: within 2^-4 of the value, relative to the group's largest
    err = (d32 - x.float()).reshape(2, 6, 2 * H, D).abs().amax(-1)
    assert (err <= x.float().reshape(2, 6, 2 * H, D).abs().amax(-1) * 2.0 ** -4).all()


def test_row_bytes():
    for H in (2, 3, 12):
        for D in (64, 128):
            R = TN.kv_fp8_row_bytes(H, D)
            assert R % 16 == 0 and 2 * H * D + 2 * H <= R < 2 * H * D + 2 * H + 16
    assert TN.kv_fp8_row_bytes(12, 64) == 1568


def _layers():
    return [SelfAttentionLayer.Builder().nIn(128).nOut(128).nHeads(2).causal(True),
            TransformerEncoderLayer.Builder().nIn(128).nOut(128).nHeads(2).ffnSize(24).causal(True),
            TransformerDecoderLayer.Builder().nIn(128).nInMemory(128).nOut(128).nHeads(2).ffnSize(24)]


def test_conf_field_round_trips_and_the_default_leaves_the_json_alone():
    for b in _layers():
        plain = b.build()
        assert plain.cacheDataType is None
        text = plain.toJson()
        assert "cacheDataType" not in text
        assert type(plain).fromJson(text) == plain
        fp8 = b.cacheDataType("fp8").build()
        text8 = fp8.toJson()
        assert json.loads(text8)["cacheDataType"] == "fp8"
        back = type(fp8).fromJson(text8)
        assert back.cacheDataType == "fp8" and back == fp8 and back != plain
        d = json.loads(text8)
        del d["cacheDataType"]
        assert json.dumps(d, indent=2, sort_keys=True) == text
        for bad in ("fp4", "bf16", 8, True):
            with pytest.raises(DL4JInvalidConfigException, match="cacheDataType"):
                b.cacheDataType(bad).build()
        b.cacheDataType(None)


def _lm_graph(dt, device, T, cache=None, V=11, E=128, H=2, F=24):
    """The two-block causal language model of tests/test_gpu_attention_decode.py, with the cache format."""
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.05)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(T + 2).inputLength(T).build(), "tokens")
    g.addLayer("enc0", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)
               .cacheDataType(cache).build(), "emb")
    g.addLayer("enc1", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)
               .cacheDataType(cache).build(), "enc0")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=device)
    return net


def test_network_conf_round_trips_and_set_cache_data_type():
    net = _lm_graph(DataType.FLOAT, CPU, 8)
    text = net.conf.toJson()
    assert "cacheDataType" not in text
    net.rnnSetCacheDataType("fp8")
    assert net.layers_by_name["enc0"].conf.cacheDataType == "fp8" == net.layers_by_name["enc1"].conf.cacheDataType
    assert net.conf.toJson().count('"cacheDataType": "fp8"') == 2
    again = ComputationGraphConfiguration.fromJson(net.conf.toJson())
    assert again.toJson() == net.conf.toJson()
    with pytest.raises(DL4JInvalidConfigException):
        net.rnnSetCacheDataType("int8")
    x = torch.randint(0, 11, (2, 3), generator=torch.Generator().manual_seed(0))
    net.rnnTimeStep(x)
    assert net.rnnGetPreviousState("enc0")["kvFormat"] == "fp8"
    with pytest.raises(DL4JInvalidInputException, match="enc0"):
        net.rnnSetCacheDataType(None)
    assert net.layers_by_name["enc1"].conf.cacheDataType == "fp8", "a refused call changes nothing"
    net.rnnClearPreviousState()
    net.rnnSetCacheDataType(None)
    assert net.conf.toJson() == text
    net.rnnTimeStep(x)
    st = net.rnnGetPreviousState("enc0")
    assert "kvFormat" not in st and st["kv"].dtype == torch.float32


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.cpu())
    dst._params_changed()


class _Emulation:
    """The fp8-cache network's rnnTimeStep written out on its parameters. The attention of a block is
    attention_decode_reference over the dequantised STORED state of that block (read back after the network's own
    step, so it holds the chunk's rows, which must equal the quantised K | V computed here), or, with ``own``, over
    the chunk's own unquantised K / V. The embeddings come from a twin network's embedding layer fed in lockstep."""

    def __init__(self, net, twin):
        self.net, self.emb = net, twin.layers_by_name["emb"]
        self.emb.rnnClearPreviousState()

    def _block(self, name, x, pos, own):
        import torch.nn.functional as F
        l = self.net.layers_by_name[name]
        p = {k: v.float() for k, v in l.params.items()}
        H = l.conf.nHeads
        mb, E, Tn = x.shape
        xt = x.permute(0, 2, 1).reshape(mb * Tn, E)
        qkv = (xt @ p["Wqkv"] + p["bqkv"]).reshape(mb, Tn, 3 * E)
        st = l.rnnGetPreviousState()
        assert st["kvFormat"] == "fp8" and st["kv"].dtype == torch.uint8
        assert st["kv"].shape == (mb, pos + Tn, TN.kv_fp8_row_bytes(H, E // H))
        stored = TN.kv_fp8_dequantize_reference(st["kv"], H, E // H, torch.float32)
        # the rows the step stored are the quantised chunk (up to fp32 summation order in the projection: compared
        # as values, a code apart at the most where a value sits on a rounding boundary)
        mine = TN.kv_fp8_dequantize_reference(TN.kv_fp8_quantize_reference(qkv[:, :, E:], H), H, E // H, torch.float32)
        assert (stored[:, pos:] - mine).abs().max() <= 0.125 * mine.abs().max()
        assert (stored[:, pos:] != mine).float().mean() < 1e-3
        kv = qkv[:, :, E:] if own else stored
        ctx = TN.attention_decode_reference(qkv[:, :, :E], kv[:, :, :E], kv[:, :, E:], H, pos).reshape(mb * Tn, E)
        eps = l.conf.layerNormEps
        h1 = F.layer_norm(ctx @ p["Wo"] + p["bo"] + xt, (E,), p["ln1g"].reshape(-1), p["ln1b"].reshape(-1), eps)
        f = F.gelu(h1 @ p["W1"] + p["b1"]) @ p["W2"] + p["b2"]
        y = F.layer_norm(f + h1, (E,), p["ln2g"].reshape(-1), p["ln2b"].reshape(-1), eps)
        return y.reshape(mb, Tn, E).permute(0, 2, 1)

    def step(self, x, pos, own=False):
        """-> (the network's output for the chunk x [mb, Tn] at ``pos``, the emulation's), both [mb, V, Tn]."""
        out = self.net.rnnTimeStep(x)[0]
        h = self.emb.rnnTimeStep(x).float()
        for name in ("enc0", "enc1"):
            h = self._block(name, h, pos, own)
        o = self.net.layers_by_name["out"]
        mb, E, Tn = h.shape
        z = h.permute(0, 2, 1).reshape(mb * Tn, E) @ o.params["W"].float() + o.params["b"].float()
        return out, torch.softmax(z, 1).reshape(mb, Tn, -1).permute(0, 2, 1)


def test_fp32_cpu_network_with_the_fp8_cache_matches_the_emulation():
    T, MB, V = 70, 2, 11
    net = _lm_graph(DataType.FLOAT, CPU, T, "fp8")
    plain, twin = _lm_graph(DataType.FLOAT, CPU, T), _lm_graph(DataType.FLOAT, CPU, T)
    _copy_params(plain, net)
    _copy_params(twin, net)
    x = torch.randint(0, V, (MB, T), generator=torch.Generator().manual_seed(0))
    ref = plain.output(x)[0]
    # token by token: every step attends over what the cache holds, its own new row included
    net.rnnClearPreviousState()
    emu = _Emulation(net, twin)
    outs = []
    for t in range(T):
        out, want = emu.step(x[:, t:t + 1], t)
        assert (out - want).abs().max() < 1e-5, t
        outs.append(out)
    seq = torch.cat(outs, 2)
    rel_q = ((seq - ref).norm() / ref.norm()).item()
    print(f"fp32 CPU, fp8 cache against the plain cache over T={T}: rel {rel_q:.3e}")
    assert 0 < rel_q < 5e-2                 # quantised, and no further off than 4 significant bits allow
    # a 66-token prompt into the empty cache attends over its own unquantised K / V and stores quantised rows; the
    # steps after it attend over the cache
    net.rnnClearPreviousState()
    emu = _Emulation(net, twin)
    out, want = emu.step(x[:, :66], 0, own=True)
    assert (out - want).abs().max() < 1e-5
    assert (out - ref[:, :, :66]).abs().max() < 1e-4, "the prompt chunk is the unquantised causal forward"
    for t in range(66, T):
        out, want = emu.step(x[:, t:t + 1], t)
        assert (out - want).abs().max() < 1e-5, t
    assert (out - ref[:, :, T - 1:]).abs().max() > 0, "the steps after the prompt read the quantised cache"
    # a chunk below 64 tokens into the empty cache attends over the cache
    net.rnnClearPreviousState()
    emu = _Emulation(net, twin)
    out, want = emu.step(x[:, :63], 0)
    assert (out - want).abs().max() < 1e-5
    assert (out - ref[:, :, :63]).abs().max() > 0


def test_state_round_trips_between_the_formats():
    T, MB = 9, 2
    fp8 = _lm_graph(DataType.FLOAT, CPU, T, "fp8")
    plain = _lm_graph(DataType.FLOAT, CPU, T)
    _copy_params(plain, fp8)
    x = torch.randint(0, 11, (MB, T), generator=torch.Generator().manual_seed(3))
    fp8.rnnTimeStep(x[:, :5])
    plain.rnnTimeStep(x[:, :5])
    for name in ("enc0", "enc1"):
        s8, s32 = fp8.rnnGetPreviousState(name), plain.rnnGetPreviousState(name)
        assert s8["kvFormat"] == "fp8" and s8["kv"].shape == (MB, 5, TN.kv_fp8_row_bytes(2, 64))
        # fp8 -> the plain layer -> values; the plain state -> the fp8 layer -> quantised rows
        plain.rnnSetPreviousState(name, s8)
        back = plain.rnnGetPreviousState(name)
        assert "kvFormat" not in back
        assert torch.equal(back["kv"], TN.kv_fp8_dequantize_reference(s8["kv"], 2, 64, torch.float32))
        fp8.rnnSetPreviousState(name, s32)
        assert torch.equal(fp8.rnnGetPreviousState(name)["kv"], TN.kv_fp8_quantize_reference(s32["kv"], 2))
        # dequantised values are representable: fp8 -> plain -> fp8 keeps every value (a group whose largest code
        # was exactly 224 comes back one exponent lower, so the bytes may differ)
        fp8.rnnSetPreviousState(name, back)
        again = TN.kv_fp8_dequantize_reference(fp8.rnnGetPreviousState(name)["kv"], 2, 64, torch.float32)
        assert torch.equal(again, back["kv"])
        fp8.rnnSetPreviousState(name, s8)
        assert torch.equal(fp8.rnnGetPreviousState(name)["kv"], s8["kv"])
