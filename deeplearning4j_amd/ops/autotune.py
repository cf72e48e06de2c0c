"""The one per-shape kernel chooser. Every autotuned decision of ``ops/conv_native.py`` and ``ops/gemm.py`` — conv
tile variant, weight-gradient engine and split count, 1x1-conv GEMM-vs-implicit-GEMM, GEMM tile x split-K, fp32
library-vs-exact kernel — is one call of ``pick``; the call's arguments are where the sites differ (probe launch,
accepted statuses, repetitions, warm-up, inline on the main stream, database table). The callers sit on the
per-launch path, so they test their memo dict themselves before they build the closures ``pick`` takes: a shape's
steady state stays one dict lookup."""
import contextlib

import torch

from . import side_stream, timing, tunedb


def capturing():
    """A HIP graph is being captured on the current stream: nothing can be timed."""
    return torch.cuda.is_current_stream_capturing()


def pick(memo, key, *, candidates, run, default, table=None, fallback=None, ok=(0,), reps=3, warmup=1,
         scale_reps=True, probe=True, inline=False, enabled=True, log=None):
    """The choice for ``key`` and whether it came from the database: ``(choice, from_db)``.

    memo hit -> tunedb hit (memoised) -> under capture or with ``enabled`` false: ``default()``, NOT memoised ->
    time every candidate, memoise and ``tunedb.record`` the fastest (the first of equal times).

    memo: the caller's module-level dict. table: the tunedb table, None for a choice that is not persisted.
    candidates(), default(): called only when needed (they may query the kernel library or allocate scratch).
    run(cand): enqueue one launch on a scratch destination, return its status. With ``probe`` a candidate whose
    first launch returns a status outside ``ok`` is skipped; when none is left ``fallback`` (``default()`` when
    None) is the choice.
    reps, warmup: ``timing.gpu_time`` arguments; ``scale_reps`` lets DL4J_AMD_TUNE_REPS raise ``reps``.
    inline: time with the weight-gradient overlap stream suspended (candidates that reach ``side_stream.run``).
    log(best, [(ms, cand)]): called after a timing pass that timed anything."""
    v = memo.get(key)
    if v is not None:
        return v, False
    if table is not None:
        v = tunedb.lookup(table, key)
        if v is not None:
            memo[key] = v
            return v, True
    if not enabled or capturing():
        return default(), False
    n = tunedb.reps(reps) if scale_reps else reps
    times = []
    with side_stream.suspended() if inline else contextlib.nullcontext():
        for cand in candidates():
            if probe and run(cand) not in ok:
                continue
            # GPU-side time (stream parked during the enqueue): small kernels are shorter than the host launch path
            times.append((timing.gpu_time(lambda: run(cand), reps=n, warmup=warmup), cand))
    if times:
        v = min(times, key=lambda tc: tc[0])[1]
        if log is not None:
            log(v, times)
    else:
        v = default() if fallback is None else fallback
    memo[key] = v
    if table is not None:
        tunedb.record(table, key, v)
    return v, False
