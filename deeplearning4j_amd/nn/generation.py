"""Token generation on top of ``rnnTimeStep``: greedy decoding, temperature / top-k / top-p sampling and beam search
for MultiLayerNetwork and ComputationGraph (``net.generate(prompt, ...)``).

Per generated token the loop runs one device op that turns the next-token distribution into a token
(ops/generation_native.py: the row sampler or the beam step of csrc/generation.hip), for beam search one
``rnnReorderState`` (the key/value-cache gather) and one ``rnnTimeStep``. The distribution is read in the network's
compute dtype, the int64 token tensor the kernel wrote is the next input as it is, and the host reads the device's
count of unfinished rows only every ``eosCheckEvery`` steps (never without an ``eosToken``): steps run past the point
where every row finished only produce ``padToken``, so the result does not depend on that interval.

Prompts of different lengths go in right-padded with ``promptLengths``: the prompt runs once on the padded rectangle,
``rnnTrimState(lengths)`` lets every cached layer continue row b at its own position (a device array of per-row
shortfalls, written once per sequence), row b's first distribution is read at time step ``lengths[b] - 1`` and the
loops run unchanged."""
import collections
import dataclasses
from typing import Optional

import torch

from ..exceptions import DL4JInvalidConfigException, DL4JInvalidInputException

GenerationResult = collections.namedtuple("GenerationResult", ["tokens", "lengths", "scores"])


@dataclasses.dataclass
class GenerationConfig:
    """maxNewTokens: tokens to generate per example. doSample: draw from the (temperature / topK / topP filtered)
    distribution instead of taking its argmax. numBeams > 1: beam search (not with doSample); a beam's final score is
    sumLogProb / length**lengthPenalty. eosToken: a row stops at it and is filled with padToken afterwards. seed: with
    it the result is a pure function of (parameters, prompt, config); None draws one from torch's generator.
    eosCheckEvery: steps between host reads of the device's unfinished count. inputEncoding: "ids" (token ids
    [mb, T]) or "onehot" ([mb, V, T], built on the device). tokenInput: for a graph, the network input that carries
    the generated stream (default: the last one)."""
    maxNewTokens: int = 16
    doSample: bool = False
    temperature: float = 1.0
    topK: int = 0
    topP: float = 1.0
    numBeams: int = 1
    lengthPenalty: float = 1.0
    eosToken: Optional[int] = None
    padToken: int = 0
    seed: Optional[int] = None
    eosCheckEvery: int = 16
    inputEncoding: str = "ids"
    tokenInput: Optional[str] = None

    def validate(self):
        def bad(msg):
            raise DL4JInvalidConfigException(f"GenerationConfig: {msg}")
        if int(self.maxNewTokens) < 1:
            bad(f"maxNewTokens must be >= 1, got {self.maxNewTokens}")
        if not 1 <= int(self.numBeams) <= 16:
            bad(f"numBeams must be in 1..16, got {self.numBeams}")
        if self.doSample and int(self.numBeams) > 1:
            bad("doSample cannot be combined with numBeams > 1")
        if not float(self.temperature) > 0.0:
            bad(f"temperature must be > 0, got {self.temperature}")
        if not 0.0 < float(self.topP) <= 1.0:
            bad(f"topP must be in (0, 1], got {self.topP}")
        if int(self.topK) < 0:
            bad(f"topK must be >= 0 (0 = off), got {self.topK}")
        if int(self.eosCheckEvery) < 1:
            bad(f"eosCheckEvery must be >= 1, got {self.eosCheckEvery}")
        if self.inputEncoding not in ("ids", "onehot"):
            bad(f'inputEncoding must be "ids" or "onehot", got {self.inputEncoding!r}')
        if self.eosToken is not None and int(self.eosToken) < 0:
            bad(f"eosToken must be >= 0 or None, got {self.eosToken}")
        return self


def _prompt_tensor(prompt, device):
    try:
        if hasattr(prompt, "toTensor"):
            prompt = prompt.toTensor()
        p = prompt if torch.is_tensor(prompt) else torch.as_tensor(prompt)
    except (ValueError, TypeError) as e:
        raise DL4JInvalidInputException(
            "generate: the prompt must be ids [mb, Tp] of one common length; ragged prompts are not supported (the "
            f"cached decode kernel takes one position for the whole batch): {e}") from None
    if p.dim() != 2 or p.shape[1] < 1 or p.shape[0] < 1 or p.is_floating_point() and bool((p != p.round()).any()):
        raise DL4JInvalidInputException(
            f"generate: the prompt must be ids [mb, Tp] of one common length, got shape {tuple(p.shape)}; ragged "
            "prompts are not supported (the cached decode kernel takes one position for the whole batch)")
    return p.to(device=device, dtype=torch.int64)


def _lengths_tensor(lengths, mb, what):
    """``lengths`` as int64 [mb] on the host (the one host read of a ragged batch)."""
    try:
        n = torch.as_tensor(lengths).detach().cpu().reshape(-1)
    except (ValueError, TypeError, RuntimeError) as e:
        raise DL4JInvalidInputException(f"{what}: lengths must be integers [{mb}]: {e}") from None
    if n.is_floating_point() or n.dtype == torch.bool or (mb is not None and n.numel() != mb):
        raise DL4JInvalidInputException(f"{what}: lengths must be integers [{mb}], got {n.dtype} {tuple(n.shape)}")
    return n.to(torch.int64)


def trim_layers(named, lengths):
    """rnnTrimState of a network over its (label, layer) pairs: the lengths are read once, every layer first only
    validates (a layer that keeps rnnTimeStep state but cannot trim it refuses), then every layer is trimmed."""
    n = _lengths_tensor(lengths, None, "rnnTrimState")
    todo = [(label, l) for label, l in named if hasattr(l, "rnnClearPreviousState")]
    for dry in (True, False):
        for label, l in todo:
            try:
                if not hasattr(l, "rnnTrimState"):
                    from .layers.recurrent import cannot_trim
                    cannot_trim(l)
                l.rnnTrimState(n, dryRun=dry)
            except DL4JInvalidInputException as e:
                raise DL4JInvalidInputException(f"{label}: {e}") from None


class _Stepper:
    """Feeds the network: the first call with the prompt (and the other inputs), then one token tensor per call.
    Every call returns the last time step's distribution [rows, V], contiguous, in the compute dtype."""

    def __init__(self, net, cfg, others, masks):
        self.net, self.cfg = net, cfg
        self.graph = hasattr(net, "layers_by_name")
        self.masks = masks
        if self.graph:
            names = list(net.conf.networkInputs)
            tin = cfg.tokenInput if cfg.tokenInput is not None else names[-1]
            if tin not in names:
                raise DL4JInvalidConfigException(f"GenerationConfig: tokenInput {tin!r} is not one of the network "
                                                 f"inputs {names}")
            others = dict(others or {})
            missing = [n for n in names if n != tin and n not in others]
            extra = [n for n in others if n not in names or n == tin]
            if missing or extra:
                raise DL4JInvalidInputException(f"generate: others must map exactly the network inputs other than "
                                                f"{tin!r} ({[n for n in names if n != tin]}); missing {missing}, "
                                                f"unexpected {extra}")
            self.names, self.tidx, self.others = names, names.index(tin), others
        elif others:
            raise DL4JInvalidInputException("generate: a MultiLayerNetwork has one input; others must be empty")
        self._hot = None

    def _encode(self, ids):
        """ids [rows, T] int64 on the device -> the network's input."""
        if self.cfg.inputEncoding == "ids":
            return ids
        V = self.vocab
        rows, T = ids.shape
        if self._hot is None or self._hot.shape != (rows, V, T):
            self._hot = torch.zeros(rows, V, T, dtype=torch.float32, device=ids.device)
        else:
            self._hot.zero_()
        return self._hot.scatter_(1, ids.reshape(rows, 1, T), 1.0)

    def _run(self, x, first, last=None):
        if self.graph:
            ins = [None] * len(self.names)
            if first:
                for i, n in enumerate(self.names):
                    if i != self.tidx:
                        ins[i] = self.others[n]
            ins[self.tidx] = x
            out = self.net._rnn_time_step_raw(*ins, masks=self.masks if first else None)[0]
        else:
            out = self.net._rnn_time_step_raw(x)
        if last is not None:                                     # ragged prompts: row b's own last time step
            return out.gather(2, last.reshape(-1, 1, 1).expand(out.shape[0], out.shape[1], 1))[:, :, 0].contiguous()
        return out[:, :, -1].contiguous() if out.dim() == 3 else out.contiguous()

    def first(self, prompt, lengths=None):
        """``lengths``: None, or int64 [mb] on the host: the prompt is right-padded and row b is that long. The
        state is trimmed to them after the prefill and row b's distribution comes from time step lengths[b] - 1."""
        if self.cfg.inputEncoding == "onehot":
            self.vocab = _vocab(self.net)
        if lengths is None:
            return self._run(self._encode(prompt), True)
        p = self._run(self._encode(prompt), True, last=(lengths - 1).to(prompt.device))
        if self.graph:
            self.net.rnnTrimState(lengths, self.names[self.tidx])
        else:
            self.net.rnnTrimState(lengths)
        return p

    def step(self, tok):
        return self._run(self._encode(tok.reshape(-1, 1)), False)


def _vocab(net):
    layer = net.layers_by_name[net.outputs[0]] if hasattr(net, "layers_by_name") else net.layers[-1]
    return int(layer.conf.nOut)


def _stream(cfg, device):
    from ..ops.nn_misc import PhiloxStream
    if cfg.seed is None:
        return PhiloxStream(device)
    s = PhiloxStream.__new__(PhiloxStream)
    s.seed = int(cfg.seed) & 0xFFFFFFFFFFFFFFFF
    s.offset = torch.zeros(1, dtype=torch.int64, device=device)
    return s


def generate(net, prompt, config=None, others=None, masks=None, useBeamPath=False, promptLengths=None,
             **configFields):
    """Generate ``maxNewTokens`` tokens per row of ``prompt`` [mb, Tp] (ids of one common length, or with
    ``promptLengths`` [mb] right-padded to Tp with row b that long, 1 <= promptLengths[b] <= Tp; the entries past a
    row's length must be valid ids and otherwise do not matter: the prompt runs as one padded rectangle, then
    ``rnnTrimState`` lets every row continue at its own position).
    ``config``: a GenerationConfig, and / or its fields as keywords. ``others``: for a graph, the remaining network
    inputs for the first call (e.g. the source of an encoder-decoder model) by name; ``masks``: as in
    ComputationGraph.rnnTimeStep, for the first call. ``useBeamPath`` runs numBeams == 1 through the beam search.
    -> GenerationResult(tokens int64 [mb, maxNewTokens], lengths int64 [mb] (up to and including eos),
    scores fp32 [mb] (the sum of the chosen tokens' log-probabilities; for beam search divided by
    length**lengthPenalty))."""
    cfg = config if config is not None else GenerationConfig()
    if configFields:
        unknown = [k for k in configFields if k not in {f.name for f in dataclasses.fields(GenerationConfig)}]
        if unknown:
            raise DL4JInvalidConfigException(f"GenerationConfig has no field(s) {unknown}")
        cfg = dataclasses.replace(cfg, **configFields)
    cfg.validate()
    prompt = _prompt_tensor(prompt, net.device)
    lengths = None
    if promptLengths is not None:
        mb, Tp = prompt.shape
        lengths = _lengths_tensor(promptLengths, mb, "generate: promptLengths")
        if int(lengths.min()) < 1 or int(lengths.max()) > Tp:
            raise DL4JInvalidInputException(
                f"generate: every prompt length must be in 1..{Tp} (the padded prompt's width), got "
                f"{lengths.tolist()}")
    stepper = _Stepper(net, cfg, others, masks)
    net.rnnClearPreviousState()
    with torch.no_grad():
        p = stepper.first(prompt, lengths)
        if int(cfg.numBeams) > 1 or useBeamPath:
            return _beam(net, stepper, p, cfg)
        return _sample(stepper, p, cfg)


def _sample(stepper, p, cfg):
    from ..ops import generation_native as GN
    mb, dev, N = p.shape[0], p.device, int(cfg.maxNewTokens)
    eos = cfg.eosToken
    tokens = torch.full((N, mb), int(cfg.padToken), dtype=torch.int64, device=dev)
    logps = torch.zeros(N, mb, dtype=torch.float32, device=dev)
    fin = count = None
    if eos is not None:
        fin = torch.zeros(mb, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = _stream(cfg, dev) if cfg.doSample else None
    for t in range(N):
        GN.sample_rows(p, cfg.temperature, cfg.topK, cfg.topP, not cfg.doSample, rng, fin, eos, cfg.padToken, count,
                       out=(tokens[t], logps[t]), advance=True)
        if t == N - 1:
            break
        if eos is not None and (t + 1) % int(cfg.eosCheckEvery) == 0 and int(count.item()) == 0:
            break
        p = stepper.step(tokens[t])
    toks = tokens.t().contiguous()
    # summed in fp64 and rounded once: a row's score does not depend on how many rows the batch has (torch's fp32
    # column sum picks its order by the shape), so a ragged batch scores every row as the row alone
    return GenerationResult(toks, _lengths(toks, eos), logps.sum(0, dtype=torch.float64).float())


def _lengths(toks, eos):
    mb, N = toks.shape
    if eos is None:
        return torch.full((mb,), N, dtype=torch.int64, device=toks.device)
    hit = toks == int(eos)
    return torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((mb,), N, device=toks.device))


def _beam(net, stepper, p, cfg):
    from ..ops import generation_native as GN
    mb, dev, N, W = p.shape[0], p.device, int(cfg.maxNewTokens), int(cfg.numBeams)
    eos = cfg.eosToken
    rows = mb * W
    # every state row becomes W rows: the prompt (and an encoder) ran once per example, not once per beam
    net.rnnReorderState(torch.arange(mb, dtype=torch.int32, device=dev).repeat_interleave(W))
    p = p.repeat_interleave(W, 0).contiguous()
    score = torch.full((mb, W), float("-inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0
    fin = torch.zeros(mb, W, dtype=torch.uint8, device=dev)
    length = torch.zeros(mb, W, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev) if eos is not None else None
    toks = torch.full((N, rows), int(cfg.padToken), dtype=torch.int64, device=dev)
    parents = torch.arange(rows, dtype=torch.int32, device=dev).repeat(N, 1)    # identity for steps never run
    for t in range(N):
        par, tok = GN.beam_step(p, score, fin, length, eos, cfg.padToken, count,
                                out=(parents[t].view(mb, W), toks[t].view(mb, W)))
        if par.data_ptr() != parents[t].data_ptr():              # the torch path returns new tensors
            parents[t].copy_(par.reshape(-1))
            toks[t].copy_(tok.reshape(-1))
        if t == N - 1:
            break
        if eos is not None and (t + 1) % int(cfg.eosCheckEvery) == 0 and int(count.item()) == 0:
            break
        net.rnnReorderState(parents[t], groupSize=W)
        p = stepper.step(toks[t])
    final = score / length.clamp(min=1).to(torch.float32) ** float(cfg.lengthPenalty)
    best = final.argmax(1)                                       # ties: the lowest beam, the better raw score
    out = GN.beam_backtrack(toks, parents, best, W)              # follow the parents back from the best beam
    bi = best.reshape(mb, 1)
    return GenerationResult(out, length.gather(1, bi).reshape(mb).to(torch.int64), final.gather(1, bi).reshape(mb))
