"""Expectations shared by tests/test_stream_active_cpu.py and tests/test_stream_active_gpu.py (not a test module): the list builder
of kws_stream_active.hip restated, and the two sets of a sparse test.  The oracle of every GPU test is a DENSE second set on a
second context: it gets the same audio on a stream while the stream is active in the sparse set, zeros while it is idle there,
and ``kws_stream_reset`` at every instant at which the sparse set activates or deactivates the stream.  The sparse set gets loud
garbage in its idle rows.  No numerical reference and no tolerance: each active stream runs the same code on the same data."""
import numpy as np

CHUNK = 1024   # RESET_CHUNK: streams per by-value mask


def mask_words(active):
    """bool [S] -> the host mirror: uint64 words, bit s % 64 of word s // 64; bits at or beyond S are clear."""
    active = np.asarray(active, bool)
    words = [0] * (-(-len(active) // 64))
    for s in np.flatnonzero(active):
        words[s >> 6] |= 1 << (int(s) & 63)
    return words


def build_list(words, n_streams):
    """The device list from the mirror, as the kernel builds it: one launch per chunk of 1024 streams that holds an active stream,
    base = the active streams of the chunks before it (host-known); thread r of a chunk, if its stream first + r is active, writes
    first + r at base + popcount(the chunk's mask bits below r).  Returns (list of n_active entries, [(first, base)] per launch)."""
    out, launches, base = {}, [], 0
    for first in range(0, n_streams, CHUNK):
        w = [words[first // 64 + k] if first // 64 + k < len(words) else 0 for k in range(CHUNK // 64)]
        n = sum(bin(x).count("1") for x in w)
        if not n:
            continue
        launches.append((first, base))
        for r in range(CHUNK):
            if first + r >= n_streams or not (w[r >> 6] >> (r & 63)) & 1:
                continue
            at = base + bin(w[r >> 6] & ((1 << (r & 63)) - 1)).count("1") + sum(bin(w[k]).count("1") for k in range(r >> 6))
            assert at not in out
            out[at] = first + r
        base += n
    assert sorted(out) == list(range(base))
    return [out[i] for i in range(base)], launches


def default_cluster(n_active):
    """stream_enqueue's rule, from the ACTIVE count."""
    return 4 if n_active <= 64 else (2 if n_active <= 128 else 1)


def active_table(S, n, plan):
    """bool [n, S]: stream s takes part in push t (0-based).  plan: {pushes so far: [(op, streams)]}, op in "activate",
    "deactivate", "reset"; every stream is active at the open."""
    on = np.ones(S, bool)
    table = np.zeros((n, S), bool)
    for t in range(n):
        for op, streams in plan.get(t, []):
            if op != "reset":
                on[list(streams)] = op == "activate"
        table[t] = on
    return table


def two_inputs(pcm, table, step, seed=7):
    """pcm int16 [S, n * step] -> (sparse set's input, dense set's input): +-32767 noise / zeros wherever the stream is idle."""
    S, n = pcm.shape[0], table.shape[0]
    idle = np.repeat(~table.T, step, axis=1)   # [S, n * step]
    noise = np.random.default_rng(seed).choice(np.array([-32767, 32767], np.int16), size=pcm.shape)
    a, b = np.array(pcm), np.array(pcm)
    a[idle] = noise[idle]
    b[idle] = 0
    return a, b


def dense_plan(plan):
    """The dense set's plan: a reset wherever the sparse set activates, deactivates or resets."""
    return {t: [("reset", streams) for _, streams in ops] for t, ops in plan.items()}
