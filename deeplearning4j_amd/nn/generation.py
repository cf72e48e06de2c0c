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
loops run unchanged.

Graph-replayed decoding (``pinPositions`` / ``useGraph``, sampling and greedy only): after the prompt
``rnnPinState(Tp + maxNewTokens)`` fixes the host's bound at the capacity and lets that device array carry the
positions, the sampler writes a staging row and the time step ends with one commit launch (``dl4j_gen_step_commit``)
that lowers every shortfall and files the staging row under a device step counter. Every step then has the same
launch arguments; ``useGraph`` runs it eagerly once, captures it into a HIP graph (nn/hipgraph.py) and replays it,
with the eos read staying on the host between replays. The graph lives for the call."""
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
    the generated stream (default: the last one). pinPositions: after the prompt the network's state is pinned
    (``rnnPinState``) so that every step has the same launch arguments: positions advance on the device, the sampler
    writes a staging row and one commit launch per step files it (not with numBeams > 1). useGraph: pinPositions, and
    the step is captured once into a HIP graph and replayed (GPU only). numDraftTokens K (0 = off, else 1..16):
    speculative decoding, K drafted tokens per round checked by the network in one chunked step (greedy or sampling
    without topK / topP; not with numBeams > 1, pinPositions or useGraph); the drafts come from the ``assistant`` of
    ``generate``, or without one from prompt lookup with n-grams of up to draftNgram (1..8) tokens."""
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
    pinPositions: bool = False
    useGraph: bool = False
    numDraftTokens: int = 0
    draftNgram: int = 3

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
        for f in ("useGraph", "pinPositions"):
            if getattr(self, f) and int(self.numBeams) > 1:
                bad(f"{f} cannot be combined with numBeams > 1 (beam search reorders the caches every step)")
        if not 0 <= int(self.numDraftTokens) <= 16:
            bad(f"numDraftTokens must be in 0..16 (0 = off), got {self.numDraftTokens}")
        if not 1 <= int(self.draftNgram) <= 8:
            bad(f"draftNgram must be in 1..8, got {self.draftNgram}")
        if int(self.numDraftTokens) > 0:
            if int(self.numBeams) > 1:
                bad("numDraftTokens cannot be combined with numBeams > 1 (speculative decoding checks one draft "
                    "sequence per row)")
            for f in ("useGraph", "pinPositions"):
                if getattr(self, f):
                    bad(f"numDraftTokens cannot be combined with {f} (a round sets the positions back, a pinned "
                        "state only advances)")
            if int(self.topK) != 0 or float(self.topP) != 1.0:
                bad(f"numDraftTokens cannot be combined with topK / topP (got topK={self.topK}, topP={self.topP}): "
                    "the residual of filtered distributions is not supported")
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


def positionable_layers(named):
    """The (label, layer) pairs that keep rnnTimeStep state; a layer among them whose state cannot be set back to an
    earlier position (LSTM family, SimpleRnn, a wrapper) refuses, naming itself, before anything is changed."""
    todo = [(label, l) for label, l in named if hasattr(l, "rnnClearPreviousState")]
    for label, l in todo:
        if not hasattr(l, "rnnSetPositions"):
            from .layers.recurrent import cannot_reposition
            _labelled(label, cannot_reposition, l)
    return todo


def set_positions(net, named, bound, short):
    """rnnSetPositions of a network over its (label, layer) pairs: every layer is validated (the layers that hold
    state must have seen one count of tokens in one number of rows, ``short`` must be int32 [mb] on the network's
    device), then every layer takes ``bound`` and the tensor ``short`` itself. Nothing is launched or read."""
    refuse_pinned(net, "rnnSetPositions")
    todo = positionable_layers(named)
    live = [(label, l, l.rnnPinInfo()) for label, l in todo if hasattr(l, "rnnPinInfo")]
    live = [(label, l, i) for label, l, i in live if i is not None]
    if torch.is_tensor(short) and live:
        dev = torch.device(net.device)
        if short.device.type != dev.type or (dev.index is not None and short.device.index != dev.index):
            raise DL4JInvalidInputException(f"rnnSetPositions: short is on {short.device}, the network on {dev}")
    for label, l, (s, m, _) in live:
        if (s, m) != live[0][2][:2]:
            raise DL4JInvalidInputException(
                f"rnnSetPositions: {label} has seen {s} tokens in {m} rows, {live[0][0]} {live[0][2][0]} in "
                f"{live[0][2][1]}; one bound and one position array cannot serve both")
    for dry in (True, False):
        for label, l in todo:
            _labelled(label, l.rnnSetPositions, bound, short, dryRun=dry)


def set_cache_data_type(named, value):
    """rnnSetCacheDataType of a network over its (label, layer) pairs: every layer whose configuration has
    ``cacheDataType`` takes ``value`` (None = the compute dtype, "fp8"). A layer that holds a key/value cache refuses,
    named, before any layer is changed: the stored rows are in the old format."""
    if value is not None and value != "fp8":
        raise DL4JInvalidConfigException(f"rnnSetCacheDataType: None (the compute dtype) or \"fp8\", got {value!r}")
    todo = [(label, l) for label, l in named if "cacheDataType" in type(l.conf)._all_fields()]
    for label, l in todo:
        if l.rnnPinInfo() is not None:
            raise DL4JInvalidInputException(
                f"rnnSetCacheDataType: {label} ({type(l.conf).__name__}) holds rnnTimeStep state; call "
                "rnnClearPreviousState() first")
    for _, l in todo:
        l.conf.cacheDataType = value


def _labelled(label, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except DL4JInvalidInputException as e:
        raise DL4JInvalidInputException(f"{label}: {e}") from None


def pinnable_layers(named):
    """The (label, layer) pairs that keep rnnTimeStep state; a layer among them that cannot be pinned (LSTM family,
    SimpleRnn, a wrapper around one) refuses, naming itself, before anything is changed."""
    todo = [(label, l) for label, l in named if hasattr(l, "rnnClearPreviousState")]
    for label, l in todo:
        if not hasattr(l, "rnnPinState"):
            from .layers.recurrent import cannot_pin
            _labelled(label, cannot_pin, l)
    return todo


def pin_layers(net, named, capacity):
    """rnnPinState of a network over its (label, layer) pairs: every layer is validated, then every layer is pinned
    to ``capacity`` with one shared device array ``short[b] = capacity - 1 - len_b`` (len_b: the tokens row b holds).
    ``net._rnn_pin`` keeps that array and the host's count of the steps left, ``capacity - max_b len_b``."""
    capacity = int(capacity)
    if net._rnn_pin is not None:
        raise DL4JInvalidInputException("rnnPinState: the state is pinned already; call rnnClearPreviousState() to "
                                        "start a new sequence")
    live = [(label, l, l.rnnPinInfo()) for label, l in pinnable_layers(named)]
    live = [(label, l, i) for label, l, i in live if i is not None]
    if not live:
        raise DL4JInvalidInputException("rnnPinState: no layer holds rnnTimeStep state; call it after the prompt has "
                                        "gone through rnnTimeStep")
    seen, mb, first = live[0][2]
    for label, l, (s, m, sh) in live:
        if (s, m, sh is None) != (seen, mb, first is None):
            raise DL4JInvalidInputException(
                f"rnnPinState: {label} has seen {s} tokens in {m} rows ({'un' if sh is None else ''}trimmed), "
                f"{live[0][0]} {seen} in {mb} ({'un' if first is None else ''}trimmed); one position array cannot "
                "serve both")
        _labelled(label, l.rnnPinState, capacity, None, dryRun=True)
    dev = net.device
    if first is None:
        longest = seen
        short = torch.full((mb,), capacity - 1 - seen, dtype=torch.int32, device=dev)
    else:
        st = torch.stack([sh.to(dev) for _, _, (_, _, sh) in live])
        differ, least = torch.stack([(st != st[0]).any().to(torch.int32), st[0].min()]).tolist()   # the one host read
        if differ:
            raise DL4JInvalidInputException("rnnPinState: the layers' per-row lengths differ; one position array "
                                            "cannot serve them all")
        longest = seen - int(least)
        short = (st[0] + (capacity - 1 - seen)).to(torch.int32).contiguous()
    for label, l, _ in live:
        l.rnnPinState(capacity, short)
    net._rnn_pin = {"short": short, "left": capacity - longest, "capacity": capacity, "record": None}


def pin_step_begin(net):
    """Before a pinned network's time step: refuse, with nothing launched, when the capacity is used up."""
    pin = net._rnn_pin
    if pin["left"] < 1:
        raise DL4JInvalidInputException(
            f"rnnTimeStep: the pinned state's capacity of {pin['capacity']} positions is used up; call "
            "rnnClearPreviousState() to start a new sequence")


def pin_step_commit(net):
    """After a pinned network's last layer: the one launch that moves every layer one position on (and files the
    staged token of a generate() call)."""
    from ..ops import generation_native as GN
    pin = net._rnn_pin
    GN.step_commit(pin["short"], pin["record"])
    pin["left"] -= 1


def refuse_pinned(net, what):
    if net._rnn_pin is not None:
        raise DL4JInvalidInputException(f"{what}: the state is pinned (rnnPinState), its positions advance on the "
                                        "device; call rnnClearPreviousState() first")


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

    def chunk(self, ids):
        """ids [rows, Tn] int64 -> every time step's distribution as [rows, Tn, V]: a view of the network's output
        where it lies (the output layer's [rows, V, Tn] is time-major memory, so a row is contiguous in V)."""
        last = _output_layer(self.net)
        last.chunkRowsInTree = True                              # this call alone: no torch copy in a round
        try:
            if self.graph:
                ins = [None] * len(self.names)
                ins[self.tidx] = self._encode(ids)
                out = self.net._rnn_time_step_raw(*ins)[0]
            else:
                out = self.net._rnn_time_step_raw(self._encode(ids))
        finally:
            last.chunkRowsInTree = False
        return out.permute(0, 2, 1)

    def set_positions(self, bound, short):
        if self.graph:
            self.net.rnnSetPositions(bound, short, self.names[self.tidx])
        else:
            self.net.rnnSetPositions(bound, short)

    def token_layers(self):
        """(label, layer) of the layers the generated stream runs through."""
        if self.graph:
            return self.net._layers_downstream(self.names[self.tidx], "generate")
        return [(f"layer {i}", l) for i, l in enumerate(self.net.layers)]

    def pin(self, capacity):
        if self.graph:
            self.net.rnnPinState(capacity, self.names[self.tidx])
        else:
            self.net.rnnPinState(capacity)


def _output_layer(net):
    return net.layers_by_name[net.outputs[0]] if hasattr(net, "layers_by_name") else net.layers[-1]


def _vocab(net):
    return int(_output_layer(net).conf.nOut)


def _stream(cfg, device):
    from ..ops.nn_misc import PhiloxStream
    if cfg.seed is None:
        return PhiloxStream(device)
    s = PhiloxStream.__new__(PhiloxStream)
    s.seed = int(cfg.seed) & 0xFFFFFFFFFFFFFFFF
    s.offset = torch.zeros(1, dtype=torch.int64, device=device)
    return s


def generate(net, prompt, config=None, others=None, masks=None, useBeamPath=False, promptLengths=None,
             assistant=None, **configFields):
    """Generate ``maxNewTokens`` tokens per row of ``prompt`` [mb, Tp] (ids of one common length, or with
    ``promptLengths`` [mb] right-padded to Tp with row b that long, 1 <= promptLengths[b] <= Tp; the entries past a
    row's length must be valid ids and otherwise do not matter: the prompt runs as one padded rectangle, then
    ``rnnTrimState`` lets every row continue at its own position).
    ``config``: a GenerationConfig, and / or its fields as keywords. ``others``: for a graph, the remaining network
    inputs for the first call (e.g. the source of an encoder-decoder model) by name; ``masks``: as in
    ComputationGraph.rnnTimeStep, for the first call. ``useBeamPath`` runs numBeams == 1 through the beam search.
    With ``pinPositions`` / ``useGraph`` the network stays pinned afterwards (``rnnClearPreviousState()`` unpins) and
    ``net.lastGenerationStats`` tells how the steps ran: {"captures", "graphReplays", "eagerSteps"}.
    Speculative decoding (``numDraftTokens`` K >= 1, see ``_speculative``): per round K tokens are drafted — by
    ``assistant``, a second MultiLayerNetwork / ComputationGraph over the same vocabulary that takes the same
    ``others`` / ``masks``, or without one by prompt lookup — and checked by ``net`` in one chunked step; greedy output
    is the plain call's, sampled output follows the network's distribution exactly.
    ``net.lastGenerationStats`` = {"rounds", "draftTokens", "acceptedTokens"}.
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
    net.lastGenerationStats = None
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
    pinned = bool(cfg.pinPositions or cfg.useGraph)
    if pinned:
        if useBeamPath:
            raise DL4JInvalidConfigException("GenerationConfig: useGraph / pinPositions cannot run the beam path")
        if cfg.useGraph and net.device.type != "cuda":
            raise DL4JInvalidConfigException(f"GenerationConfig: useGraph needs a GPU, the network is on "
                                             f"{net.device}; pinPositions runs the same steps eagerly on any device")
        pinnable_layers(stepper.token_layers())                  # refused before the prompt runs
    K = int(cfg.numDraftTokens)
    drafter = None
    if assistant is not None and K == 0:
        raise DL4JInvalidConfigException("generate: an assistant drafts for speculative decoding, which "
                                         "numDraftTokens >= 1 turns on; got numDraftTokens=0")
    if K > 0:
        if useBeamPath:
            raise DL4JInvalidConfigException("GenerationConfig: numDraftTokens cannot run the beam path")
        if assistant is net:
            raise DL4JInvalidInputException("generate: the assistant must be a network of its own (a clone of the "
                                            "network, not the network itself): both keep rnnTimeStep state")
        if assistant is not None:
            drafter = _Stepper(assistant, cfg, others, masks)
        _speculative_check(stepper, drafter, prompt.shape[1], cfg)   # refused before the prompt runs
        if assistant is not None:
            assistant.rnnClearPreviousState()
    net.rnnClearPreviousState()
    with torch.no_grad():
        p = stepper.first(prompt, lengths)
        if K > 0:
            return _speculative(net, stepper, drafter, p, cfg, prompt, lengths)
        if int(cfg.numBeams) > 1 or useBeamPath:
            return _beam(net, stepper, p, cfg)
        if pinned:
            try:
                return _sample_pinned(net, stepper, p, cfg, prompt.shape[1])
            finally:
                if net._rnn_pin is not None:
                    net._rnn_pin["record"] = None                # the call's buffers are not the network's to keep
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


def _speculative_check(stepper, drafter, Tp, cfg):
    """What speculative decoding needs of the network(s), checked before the prompt runs: one vocabulary, state that
    rnnSetPositions can set back, and position tables that hold a chunk which overshoots the last position by K."""
    N, K = int(cfg.maxNewTokens), int(cfg.numDraftTokens)
    roles = [("the network", stepper)] + ([("the assistant", drafter)] if drafter is not None else [])
    if drafter is not None and _vocab(drafter.net) != _vocab(stepper.net):
        raise DL4JInvalidInputException(
            f"generate: the assistant's vocabulary has {_vocab(drafter.net)} tokens, the network's "
            f"{_vocab(stepper.net)}; speculative decoding needs one vocabulary")
    for role, s in roles:
        _labelled(f"generate: {role}", positionable_layers, s.token_layers())
        limits = [l.rnnPinLimit() for _, l in s.token_layers() if hasattr(l, "rnnPinLimit")]
        limit = min([n for n in limits if n is not None], default=None)
        if limit is not None and Tp + N + K > limit:
            raise DL4JInvalidInputException(
                f"generate: {role} holds {limit} positions, fewer than the prompt's {Tp} + maxNewTokens {N} + "
                f"numDraftTokens {K} (a round's chunk may overshoot the last position by numDraftTokens)")


def _speculative(net, stepper, drafter, p, cfg, prompt, lengths):
    """Speculative decoding: the first token comes from the row sampler on the prompt's distribution; then per round
    K tokens are drafted (``drafter``: K + 1 single steps of the assistant, the row sampler drawing d_(i+1) from each
    of the first K outputs, which are kept; the last step only fills the assistant's cache row, so both networks hold
    the same K + 1 new rows — or one prompt-lookup launch), the network takes the chunk [next, d_1 .. d_K] in one
    step, the verify launch emits every row's accepted drafts and one more token, the commit launch turns the rows'
    new lengths into one shortfall array, and the host reads two integers (rows not finished, the longest row) — the
    round's only device-to-host copy — and sets both networks' positions to them. Rejected drafts cost nothing to
    take back: their cache rows lie past the row's position and the next chunk overwrites them. Finished rows ride
    along at their frozen position."""
    from ..ops import generation_native as GN
    mb, dev, N, K = p.shape[0], p.device, int(cfg.maxNewTokens), int(cfg.numDraftTokens)
    Tp, eos, pad, greedy = prompt.shape[1], cfg.eosToken, int(cfg.padToken), not cfg.doSample
    stats = {"rounds": 0, "draftTokens": 0, "acceptedTokens": 0}
    net.lastGenerationStats = stats
    rng = _stream(cfg, dev) if cfg.doSample else None
    fin = torch.zeros(mb, dtype=torch.uint8, device=dev)
    tm = torch.zeros(K + 1, mb, dtype=torch.int64, device=dev)   # row 0: the next input; 1 .. K: an assistant's drafts
    lp = torch.zeros(mb, dtype=torch.float32, device=dev)
    GN.sample_rows(p, cfg.temperature, 0, 1.0, greedy, rng, fin, eos, pad, None, out=(tm[0], lp), advance=True)
    tokens = torch.full((mb, N), pad, dtype=torch.int64, device=dev)
    logps = torch.zeros(mb, N, dtype=torch.float32, device=dev)
    tokens[:, 0] = tm[0]
    logps[:, 0] = lp
    if N > 1:
        length = torch.full((mb,), Tp, dtype=torch.int32, device=dev) if lengths is None else \
            lengths.to(device=dev, dtype=torch.int32)
        cursor = torch.ones(mb, dtype=torch.int32, device=dev)
        chunk = torch.zeros(mb, K + 1, dtype=torch.int64, device=dev)
        chunk[:, 0] = tm[0]
        short = torch.zeros(mb, dtype=torch.int32, device=dev)
        slot = torch.zeros(2, dtype=torch.int32, device=dev)
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        hist = qbuf = None
        if drafter is None:
            hist = torch.zeros(mb, Tp + N, dtype=torch.int64, device=dev)
            hist[:, :Tp] = prompt
            hist.scatter_(1, length.to(torch.int64).reshape(mb, 1), tm[0].reshape(mb, 1))
        else:
            drafter.first(prompt, lengths)
            qbuf = torch.empty(K, mb, p.shape[1], dtype=p.dtype, device=dev)
        GN.spec_commit(length, fin, short, slot)
        while True:
            unfinished, bound = slot.tolist()                    # the one host read of a round
            stepper.set_positions(bound, short)
            if drafter is not None:
                drafter.set_positions(bound, short)
            if unfinished == 0:
                break
            if drafter is None:
                GN.ngram_draft(hist, length, cfg.draftNgram, K, chunk[:, 1:])
            else:
                for i in range(K):
                    q = drafter.step(tm[i])
                    GN.sample_rows(q, cfg.temperature, 0, 1.0, greedy, rng, None, None, pad, None,
                                   out=(tm[i + 1], lp), advance=True)
                    GN.spec_keep(q, qbuf[i], tm[i + 1], chunk[:, i + 1])
                drafter.step(tm[K])
            GN.spec_verify(stepper.chunk(chunk), None if drafter is None else qbuf.permute(1, 0, 2), chunk[:, 1:],
                           cfg.temperature, greedy, rng, length, cursor, fin, eos, pad, tokens, logps, tm[0],
                           chunk[:, 0], hist, counters)
            GN.spec_commit(length, fin, short, slot)
            stats["rounds"] += 1
        stats["draftTokens"], stats["acceptedTokens"] = counters.tolist()
    return GenerationResult(tokens, _lengths(tokens, eos), logps.sum(1, dtype=torch.float64).float())


def _pin_capacity(stepper, Tp, N):
    """Tp + N positions; one less (the last token is sampled, never fed) where a position table ends there."""
    limits = [l.rnnPinLimit() for _, l in stepper.token_layers() if hasattr(l, "rnnPinLimit")]
    limit = min([n for n in limits if n is not None], default=None)         # None: a layer without a position table
    return Tp + N - 1 if limit is not None and limit == Tp + N - 1 else Tp + N


def _sample_pinned(net, stepper, p, cfg, Tp):
    """``_sample`` with constant launch arguments per step: the state is pinned, the sampler reads the static
    distribution buffer and writes the staging row, the time step runs on the staged token and its commit launch
    lowers the shortfalls and files the staging row as row ``t`` of the results. With ``useGraph`` that body runs
    eagerly once (autotuning, workspaces and the one-hot buffer settle), is captured once and replayed; the last
    token takes the sampler and the commit alone, eagerly."""
    from ..ops import generation_native as GN
    mb, dev, N = p.shape[0], p.device, int(cfg.maxNewTokens)
    eos = cfg.eosToken
    stepper.pin(_pin_capacity(stepper, Tp, N))
    pin = net._rnn_pin
    tokens = torch.full((N, mb), int(cfg.padToken), dtype=torch.int64, device=dev)
    logps = torch.zeros(N, mb, dtype=torch.float32, device=dev)
    stok = torch.zeros(mb, dtype=torch.int64, device=dev)
    slogp = torch.zeros(mb, dtype=torch.float32, device=dev)
    record = (torch.zeros(1, dtype=torch.int32, device=dev), stok, slogp, tokens, logps)
    pin["record"] = record
    fin = count = None
    if eos is not None:
        fin = torch.zeros(mb, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = _stream(cfg, dev) if cfg.doSample else None
    pbuf = p.clone()
    stats = {"captures": 0, "graphReplays": 0, "eagerSteps": 0}
    net.lastGenerationStats = stats

    def sample():
        GN.sample_rows(pbuf, cfg.temperature, cfg.topK, cfg.topP, not cfg.doSample, rng, fin, eos, cfg.padToken,
                       count, out=(stok, slogp), advance=True)

    def body():
        sample()
        pbuf.copy_(stepper.step(stok))

    graph = None
    for t in range(N - 1):
        if cfg.useGraph and graph is None and t >= 1:
            graph = _capture_step(net, body)
            pin["left"] += 1                                     # capturing ran the host's count, not the step
            stats["captures"] += 1
        if graph is not None:
            pin_step_begin(net)
            graph.replay()
            pin["left"] -= 1
            stats["graphReplays"] += 1
        else:
            body()
            stats["eagerSteps"] += 1
        if eos is not None and (t + 1) % int(cfg.eosCheckEvery) == 0 and int(count.item()) == 0:
            break
    else:
        sample()
        GN.step_commit(None, record)
        stats["eagerSteps"] += 1
    if graph is not None:
        torch.cuda.current_stream(dev).synchronize()             # the graph and its pool go with this call
    toks = tokens.t().contiguous()
    return GenerationResult(toks, _lengths(toks, eos), logps.sum(0, dtype=torch.float64).float())


def _capture_step(net, body):
    from . import hipgraph
    g = torch.cuda.CUDAGraph()
    with hipgraph.capture_gc_guard():
        hipgraph.capture(g, torch.cuda.graph_pool_handle(), body, net.device)
    return g


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
