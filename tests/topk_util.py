"""Shared by the top-K tests (context option "top_k"): the float64 reference of a
row's alternatives, the checks every returned (ids, logprobs) pair must pass,
and a small GGUF v3 header reader used to write a model copy whose embedding
has duplicated rows (equal logits in chosen columns)."""
import shutil
import struct

import numpy as np

SELF_BAR = 2e-5    # against float64 of the same call's logits (tests/test_gpu_logprobs.py)
PATH_BAR = 4e-5    # between two paths over bit-identical logits


def topk_ref(logits, K):
    """np.argsort(-logits, kind="stable")[:K] without sorting the whole row: the
    columns at or above the K-th largest value, stably sorted"""
    v = np.asarray(logits)
    kth = np.partition(v, len(v) - K)[len(v) - K]
    cand = np.flatnonzero(v >= kth)
    return cand[np.argsort(-v[cand], kind="stable")][:K]


def logsoftmax64(logits):
    v = np.asarray(logits, np.float64)
    m = v.max()
    return v - (m + np.log(np.exp(v - m).sum()))


def check_rows(logits, am, ids, lps, K):
    """every row of one step: ids exact against its own logits, values within
    SELF_BAR of float64 and non-increasing, entry 0 the call's argmax.  Returns
    the largest |value - float64 value|."""
    worst = 0.0
    assert ids.shape == lps.shape == (len(am), K), (ids.shape, lps.shape)
    for b in range(len(am)):
        ref = topk_ref(logits[b], K)
        if b == 0:   # the shortcut is the definition: one whole-row stable argsort a step
            assert np.array_equal(ref, np.argsort(-np.asarray(logits[b]), kind="stable")[:K])
        assert np.array_equal(ids[b], ref), (b, ids[b], ref)
        assert ids[b, 0] == am[b], (b, ids[b], am[b])
        assert (np.diff(lps[b]) <= 0).all(), (b, lps[b])
        ls = logsoftmax64(logits[b])
        worst = max(worst, float(np.abs(lps[b].astype(np.float64) - ls[ref]).max()))
    assert worst <= SELF_BAR, worst
    return worst


# ------------------------------------------------------------- GGUF v3 header
_SCALAR = {0: "B", 1: "b", 2: "H", 3: "h", 4: "I", 5: "i", 6: "f", 7: "?", 10: "Q", 11: "q", 12: "d"}


def _value(f, t):
    if t in _SCALAR:
        return struct.unpack("<" + _SCALAR[t], f.read(struct.calcsize(_SCALAR[t])))[0]
    if t == 8:
        return f.read(struct.unpack("<Q", f.read(8))[0])
    if t == 9:
        et, n = struct.unpack("<IQ", f.read(12))
        return [_value(f, et) for _ in range(n)]
    raise ValueError(f"GGUF value type {t}")


def gguf_tensor(path, name):
    """(absolute byte offset, dims, ggml type) of tensor `name` in a GGUF v3 file"""
    with open(path, "rb") as f:
        magic, version, n_tensors, n_kv = struct.unpack("<4sIQQ", f.read(24))
        assert magic == b"GGUF" and version == 3, (magic, version)
        align = 32
        for _ in range(n_kv):
            key = _value(f, 8)
            val = _value(f, struct.unpack("<I", f.read(4))[0])
            if key == b"general.alignment":
                align = int(val)
        found = None
        for _ in range(n_tensors):
            tn = _value(f, 8)
            nd = struct.unpack("<I", f.read(4))[0]
            dims = struct.unpack(f"<{nd}Q", f.read(8 * nd))
            typ, off = struct.unpack("<IQ", f.read(12))
            if tn == name.encode():
                found = (off, dims, typ)
        data = (f.tell() + align - 1) // align * align
    assert found is not None, name
    return data + found[0], found[1], found[2]


def write_tied_copy(src, dst, t):
    """dst = src with token_embd.weight (f16 [vocab][hidden]) rows t + 1, t + 16 and
    (t + vocab / 2) % vocab byte copies of row t; returns the four ids ascending"""
    off, dims, typ = gguf_tensor(src, "token_embd.weight")
    assert typ == 1 and len(dims) == 2, (typ, dims)   # GGML_TYPE_F16
    hidden, vocab = int(dims[0]), int(dims[1])
    targets = [t + 1, t + 16, (t + vocab // 2) % vocab]
    assert all(0 <= x < vocab for x in targets) and len({t, *targets}) == 4, (t, targets)
    shutil.copyfile(src, dst)
    with open(dst, "r+b") as f:
        f.seek(off + t * hidden * 2)
        row = f.read(hidden * 2)
        for x in targets:
            f.seek(off + x * hidden * 2)
            f.write(row)
    return sorted([t] + targets)
