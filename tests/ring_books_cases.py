"""The cases of the replay memories' circular buffer (csrc/ring_books.h) and the model they are held to: a collections.deque(maxlen=cap)
of sequence numbers and an unclamped batch counter, which is the reference's MemoryBuffer (src/memory.jl:34-87: a CircularBuffer and
cur_batch_size, clamped only where it is read).  tests/test_ring_books_cpu.py replays them through the header alone,
tests/test_ring_books_gpu.py through both device memories.

A script is a list of ("push", n, advance) | ("new_batch",) | ("empty",).  advance = True is a trace push (push_trace!: cur_batch_size
+= n), False a push of samples (push!(mem.buf, e): the counter stays)."""
from collections import deque

T, S = True, False

# name -> (cap, script); every cap <= 8, so the device test can run them all
CASES = {
    "cap-1": (1, [("push", 1, T), ("push", 1, S), ("push", 3, T), ("push", 1, S)]),
    "fill-to-exactly-cap": (5, [("push", 2, T), ("push", 3, T)]),
    "wrap-by-one": (5, [("push", 5, T), ("push", 1, T)]),
    "total-a-multiple-of-cap-after-a-wrap": (4, [("push", 3, T), ("push", 5, S)]),
    "one-push-of-cap-plus-1": (5, [("push", 2, T), ("push", 6, S)]),
    "one-trace-of-cap-plus-1": (5, [("push", 2, S), ("push", 6, T)]),
    "one-push-of-3cap-plus-2": (3, [("push", 2, T), ("push", 11, S)]),
    "one-trace-of-3cap-plus-2": (3, [("push", 2, T), ("push", 11, T)]),
    "batch-outgrows-len": (4, [("push", 3, T), ("push", 3, T)]),
    "trace-then-samples": (8, [("push", 3, T), ("push", 2, S)]),
    "samples-push-the-batch-out": (6, [("push", 4, T), ("push", 5, S)]),
    "new-batch-between-traces": (6, [("push", 4, T), ("new_batch",), ("push", 3, T)]),
    "new-batch-then-samples-only": (6, [("push", 4, T), ("new_batch",), ("push", 3, S)]),
    "empty-then-pushes": (4, [("push", 6, T), ("empty",), ("push", 2, T), ("push", 1, S)]),
    "empty-then-wrap": (3, [("push", 2, T), ("empty",), ("push", 2, S), ("push", 2, T)]),
    "nothing-pushed": (7, []),
}
# what a case is about, where that is one figure: the (pos, run) pieces that read the whole content, the reported and the stored batch
EXPECT = {
    "cap-1": {"runs": [(0, 1)], "len": 1, "batch": 1, "stored_batch": 4},
    "fill-to-exactly-cap": {"runs": [(0, 5)], "len": 5, "batch": 5},
    "wrap-by-one": {"runs": [(1, 4), (0, 1)], "len": 5},
    "total-a-multiple-of-cap-after-a-wrap": {"runs": [(0, 4)], "len": 4},
    "one-push-of-cap-plus-1": {"skips": [0, 1], "runs": [(3, 2), (0, 3)]},
    "one-push-of-3cap-plus-2": {"skips": [0, 8], "runs": [(1, 2), (0, 1)]},
    "batch-outgrows-len": {"len": 4, "batch": 4, "stored_batch": 6},
    "trace-then-samples": {"batch": 3, "last_batch": [2, 3, 4]},
    "samples-push-the-batch-out": {"batch": 4, "stored_batch": 4, "last_batch": [5, 6, 7, 8]},
    "new-batch-then-samples-only": {"batch": 0, "last_batch": []},
    "empty-then-pushes": {"experience": [0, 1, 2], "batch": 2, "last_batch": [1, 2], "runs": [(0, 3)]},
    "nothing-pushed": {"runs": [], "len": 0, "batch": 0},
}
# CPU only: a ring as large as the API allows, far into its life.  ("set", total, cur_batch) puts the books there directly.
BIG_CAP = (1 << 31) - 1
BIG = [("set", (1 << 40) + 3, (1 << 33) + 1), ("push", 5, T), ("push", 3 * BIG_CAP + 2, S)]


def model(cap, script):
    """Replays `script`.  Returns a dict: experience (the deque, oldest first: sequence numbers since the last empty), tags (the same
    entries numbered since the START of the script, so that entries from before an empty cannot pass for new ones), len, stored_batch,
    batch (clamped), last_batch, total, and per push its skip: how many of its entries the deque no longer holds right after it."""
    buf, cur, total, base, skips = deque(maxlen=cap), 0, 0, 0, []
    for op in script:
        if op[0] == "push":
            _, n, advance = op
            buf.extend(range(total, total + n))
            skips.append(n - sum(1 for q in buf if q >= total))
            total += n
            if advance:
                cur += n
        elif op[0] == "new_batch":
            cur = 0
        elif op[0] == "empty":
            buf.clear()
            base, total, cur = base + total, 0, 0
        else:
            raise ValueError(op)
    exp = list(buf)
    batch = min(cur, len(exp))
    return {"experience": exp, "tags": [base + q for q in exp], "base": base, "len": len(exp), "stored_batch": cur, "batch": batch,
            "last_batch": exp[len(exp) - batch:], "total": total, "skips": skips}
