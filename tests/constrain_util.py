"""The decoding-constraint rule of DESIGN.md §5.6 restated in numpy, and a ctypes binding of the kernel harness
qasr_kt_constrain (include/qasr_capi.h, csrc/kernel_harness.hip).  Every step of the rule is one correctly
rounded fp32 operation or a comparison, so the restatement is exact: the kernels are held to it bit for bit and
no tolerance appears anywhere.

    l' = l                                                       the row's raw fp32 logits, l[0 .. n_valid)
    1. p != 1:  for every distinct v among h[max(0, t - w') .. t), w' = w or t:
                    l'[v] = l[v] * inv_p  if l[v] > 0  else  l[v] * p          (inv_p = fp32(1) / fp32(p))
    2. for every (id, b) of the bias list:  l'[id] = l'[id] + b
    3. n >= 1 and t >= n - 1:  for every i in 0 .. t - n with h[i .. i + n - 1) == h[t - n + 1 .. t):
                    l'[h[i + n - 1]] = -inf
    4. token = the column with the largest argmax_key(l'[j], j): larger value first, equal values by lower id
"""
import ctypes as C

import numpy as np

f32 = np.float32
NGRAM_MAX, BIAS_MAX = 8, 1024


# ------------------------------------------------------------------ the rule
def argmax_key(v, idx):
    """the engine's 64-bit key (csrc/dev_common.h): the fp32 bits made monotone, then 2^32 - 1 - column"""
    u = np.asarray(v, f32).view(np.uint32).astype(np.uint64)
    u = np.where(u >> np.uint64(31), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx, np.uint64))


def select(l):
    l = np.asarray(l, f32)
    return int(np.argmax(argmax_key(l, np.arange(len(l)))))


def banned(h, n):
    """step 3's columns for history h (t = len(h))"""
    h = [int(x) for x in h]
    t = len(h)
    if n < 1 or t < n - 1:
        return set()
    suf = h[t - n + 1:t]
    return {h[i + n - 1] for i in range(0, t - n + 1) if h[i:i + n - 1] == suf}


def apply(l, h, n=0, p=1.0, w=0, bias=None):
    """(l', token, E) for one row: l raw fp32 logits [n_valid], h the history, bias a list of (id, value) or a dict"""
    l = np.asarray(l, f32)
    out = l.copy()
    h = [int(x) for x in h]
    t = len(h)
    E = set()
    p32 = f32(p)
    with np.errstate(invalid="ignore", over="ignore"):
        if p32 != f32(1):
            inv_p = f32(1) / p32
            ww = w if w else t
            for v in sorted(set(h[max(0, t - ww):t])):
                out[v] = l[v] * inv_p if l[v] > 0 else l[v] * p32
                E.add(v)
        items = list(bias.items()) if isinstance(bias, dict) else list(bias or [])
        assert len({int(i) for i, _ in items}) == len(items), "bias ids must be distinct"
        for i, b in items:
            out[int(i)] = out[int(i)] + f32(b)
            E.add(int(i))
    for v in banned(h, n):
        out[v] = -np.inf
        E.add(v)
    return out, select(out), E


def repeats_ngram(tokens, n):
    """whether some n-gram occurs twice in tokens"""
    seen = set()
    for i in range(len(tokens) - n + 1):
        g = tuple(tokens[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False


# ------------------------------------------------------------------ binding
_P = C.c_void_p
GUARD = 3


class ConstrainCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "ld", "n_valid", "src_div", "slices", "guard", "launches", "hist_stride", "t",
                                         "no_repeat_ngram")] + [
        ("repetition_penalty", C.c_float), ("penalty_last_n", C.c_int32), ("n_bias", C.c_int32)] + [
        (n, _P) for n in ("bias_ids", "bias", "logits", "greedy", "hist", "tok", "hist_slot", "logits_out", "skey_out",
                          "flag_out")] + [
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def _fn():
    import qasr
    L = qasr.lib()
    L.qasr_kt_constrain.argtypes = [C.c_int, C.POINTER(ConstrainCall)]
    L.qasr_kt_constrain.restype = C.c_int
    return L


def _body(buf, R, what):
    raw = buf.reshape(len(buf), -1).view(np.uint32)
    assert (raw[:GUARD] == 0xFFFFFFFF).all() and (raw[GUARD + R:] == 0xFFFFFFFF).all(), f"{what}: guard entries overwritten"
    return buf[GUARD:GUARD + R]


def run_constrain(logits, greedy, hist, t, n=0, p=1.0, w=0, bias=None, n_valid=0, src_div=1, slices=0, launches=1):
    """logits fp32 [R / src_div][ld], hist int32 [R][hist_stride] -> (tok [R], edited logits [R / src_div][ld], flags
    [R / src_div], tag); checks the guards, the history slot, the untouched history and the scratch at rest"""
    L = _fn()
    logits = np.ascontiguousarray(logits, f32)
    hist = np.ascontiguousarray(hist, np.int32)
    RS, ld = logits.shape
    R, HS = hist.shape
    assert R == RS * src_div
    greedy = np.ascontiguousarray(greedy, np.int32)
    items = list(bias.items()) if isinstance(bias, dict) else list(bias or [])
    ids = np.array([i for i, _ in items] or [0], np.int32)
    val = np.array([b for _, b in items] or [0], f32)
    tok, slot = np.zeros(R + 2 * GUARD, np.int32), np.zeros(R + 2 * GUARD, np.int32)
    out = np.zeros((RS + 2 * GUARD, ld), f32)
    skey, flag = np.ones(RS, np.uint64), np.ones(RS, np.int32)
    c = ConstrainCall(R=R, ld=ld, n_valid=n_valid or ld, src_div=src_div, slices=slices, guard=GUARD, launches=launches,
                      hist_stride=HS, t=t, no_repeat_ngram=n, repetition_penalty=float(p), penalty_last_n=w, n_bias=len(items))
    for name, x in (("bias_ids", ids), ("bias", val), ("logits", logits), ("greedy", greedy), ("hist", hist), ("tok", tok),
                    ("hist_slot", slot), ("logits_out", out), ("skey_out", skey), ("flag_out", flag)):
        setattr(c, name, x.ctypes.data_as(_P))
    rc = L.qasr_kt_constrain(0, C.byref(c))
    assert rc == 0, L.qasr_last_error().decode(errors="replace")
    assert not c.declined, c.msg.decode()
    out_tok = _body(tok, R, "tok").copy()
    assert (slot[GUARD:GUARD + R] == out_tok).all(), "the history slot differs from the tokens"
    assert (slot[:GUARD] == -1).all() and (slot[GUARD + R:] == -1).all()
    assert (skey == 0).all() and (flag == 0).all(), "the scratch was not re-armed"
    return out_tok, _body(out, RS, "logits").copy(), c.tag.decode()


def check_rows(logits, greedy, hist, t, tok, edited, n_valid=0, src_div=1, **rule):
    """the harness' outputs against the rule, bit for bit; returns per logits row whether g was in E"""
    logits = np.asarray(logits, f32)
    RS, ld = logits.shape
    nv = n_valid or ld
    hit = []
    for q in range(RS):
        want, wtok, E = apply(logits[q, :nv], hist[q * src_div, :t], **rule)
        got = edited[q]
        assert (got[:nv].view(np.uint32) == want.view(np.uint32)).all(), \
            f"row {q}: edited logits differ at columns {np.flatnonzero(got[:nv].view(np.uint32) != want.view(np.uint32))[:8]}"
        assert (got[nv:].view(np.uint32) == logits[q, nv:].view(np.uint32)).all(), f"row {q}: a column past n_valid changed"
        out = np.setdiff1d(np.arange(nv), np.fromiter(E, int, len(E)))
        assert (got[out].view(np.uint32) == logits[q, out].view(np.uint32)).all(), f"row {q}: a column outside E changed"
        assert (tok[q * src_div:(q + 1) * src_div] == wtok).all(), f"row {q}: tokens {tok[q * src_div:(q + 1) * src_div]}, the rule's {wtok}"
        hit.append(int(greedy[q]) in E)
    return hit
