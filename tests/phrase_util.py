"""The hotword rule of DESIGN.md §5.7 restated in numpy, brute force over every (phrase, position) pair, and a
ctypes binding of the kernel harness qasr_kt_phrases (include/qasr_capi.h, csrc/kernel_harness.hip).  As in
tests/constrain_util.py every step is one correctly rounded fp32 operation or a comparison, so the restatement is
exact and no tolerance appears anywhere.

    phrases ph_k[0 .. len_k) with boosts b_k; a row with history h[0 .. t)
    (k, j), 0 <= j < len_k, matches when j <= t and h[t - j .. t) == ph_k[0 .. j)            (j = 0 always does)
    bonus(x) = max of b_k over the matching (k, j) with ph_k[j] == x
    steps 1 and 2 of §5.6, then   2b. l'[x] = l'[x] + bonus(x)   for every x with a bonus,   then steps 3 and 4
"""
import ctypes as C

import numpy as np

import constrain_util as cu

f32 = np.float32
PHRASE_MAX, PHRASE_LEN_MAX = 4096, 16
GUARD = cu.GUARD
_P = C.c_void_p


# ------------------------------------------------------------------ the rule
def split(phrases, boost=5.0):
    """[(ids, boost)] from a list of id lists or (ids, boost) pairs"""
    out = []
    for ph in phrases or ():
        if isinstance(ph, tuple) and len(ph) == 2 and not isinstance(ph[0], (int, np.integer)):
            out.append(([int(x) for x in ph[0]], float(ph[1])))
        else:
            out.append(([int(x) for x in ph], float(boost)))
    return out


def bonuses(phrases, h):
    """{token: bonus} for history h; also the deepest matching position j over all phrases"""
    h = [int(x) for x in h]
    t = len(h)
    got, deepest = {}, 0
    for ids, b in split(phrases):
        for j in range(len(ids)):
            if j <= t and h[t - j:t] == ids[:j]:
                b32 = f32(b)
                got[ids[j]] = max(got.get(ids[j], b32), b32)
                deepest = max(deepest, j)
    return got, deepest


def apply(l, h, phrases=None, n=0, p=1.0, w=0, bias=None):
    """(l', token, E) for one row: steps 1 and 2 through constrain_util.apply, then 2b, then the ban"""
    l = np.asarray(l, f32)
    out, _, E = cu.apply(l, h, n=0, p=p, w=w, bias=bias)
    E = set(E)
    bon, _ = bonuses(phrases, h)
    with np.errstate(invalid="ignore", over="ignore"):
        for x, b in bon.items():
            if x < len(out):
                out[x] = out[x] + f32(b)
                E.add(x)
    for v in cu.banned(h, n):
        out[v] = -np.inf
        E.add(v)
    return out, cu.select(out), E


# ------------------------------------------------------------------ binding
class PhraseCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "ld", "n_valid", "src_div", "slices", "guard", "launches", "hist_stride", "t",
                                         "no_repeat_ngram")] + [
        ("repetition_penalty", C.c_float), ("penalty_last_n", C.c_int32), ("n_bias", C.c_int32)] + [
        (n, _P) for n in ("bias_ids", "bias", "logits", "greedy", "hist", "tok", "hist_slot", "logits_out", "skey_out",
                          "flag_out")] + [
        ("n_phrases", C.c_int32), ("ph_ids", _P), ("ph_len", _P), ("ph_boost", _P), ("scanned_out", _P),
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def _fn():
    import qasr
    L = qasr.lib()
    L.qasr_kt_phrases.argtypes = [C.c_int, C.POINTER(PhraseCall)]
    L.qasr_kt_phrases.restype = C.c_int
    return L


def flat(phrases):
    ph = split(phrases)
    ids = np.array([x for i, _ in ph for x in i] or [0], np.int32)
    ln = np.array([len(i) for i, _ in ph] or [0], np.int32)
    val = np.array([b for _, b in ph] or [0], f32)
    return len(ph), ids, ln, val


def run_phrases(logits, greedy, hist, t, phrases, n=0, p=1.0, w=0, bias=None, n_valid=0, src_div=1, slices=0, launches=1):
    """constrain_util.run_constrain with a phrase list -> (tok [R], edited logits [R / src_div][ld], scanned [R / src_div]:
    the row took the scan, tag); checks the guards, the history slot, the untouched history and the scratch at rest"""
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
    n_ph, ph_ids, ph_len, ph_boost = flat(phrases)
    tok, slot = np.zeros(R + 2 * GUARD, np.int32), np.zeros(R + 2 * GUARD, np.int32)
    out = np.zeros((RS + 2 * GUARD, ld), f32)
    skey, flag, scanned = np.ones(RS, np.uint64), np.ones(RS, np.int32), np.full(RS, -2, np.int32)
    c = PhraseCall(R=R, ld=ld, n_valid=n_valid or ld, src_div=src_div, slices=slices, guard=GUARD, launches=launches,
                   hist_stride=HS, t=t, no_repeat_ngram=n, repetition_penalty=float(p), penalty_last_n=w, n_bias=len(items),
                   n_phrases=n_ph)
    for name, x in (("bias_ids", ids), ("bias", val), ("logits", logits), ("greedy", greedy), ("hist", hist), ("tok", tok),
                    ("hist_slot", slot), ("logits_out", out), ("skey_out", skey), ("flag_out", flag), ("ph_ids", ph_ids),
                    ("ph_len", ph_len), ("ph_boost", ph_boost), ("scanned_out", scanned)):
        setattr(c, name, x.ctypes.data_as(_P))
    rc = L.qasr_kt_phrases(0, C.byref(c))
    assert rc == 0, L.qasr_last_error().decode(errors="replace")
    assert not c.declined, c.msg.decode()
    out_tok = cu._body(tok, R, "tok").copy()
    assert (slot[GUARD:GUARD + R] == out_tok).all(), "the history slot differs from the tokens"
    assert (slot[:GUARD] == -1).all() and (slot[GUARD + R:] == -1).all()
    assert (skey == 0).all() and (flag == 0).all(), "the scratch was not re-armed"
    assert ((scanned == 0) | (scanned == 1)).all(), f"scanned_out {scanned}"
    return out_tok, cu._body(out, RS, "logits").copy(), scanned.astype(bool).tolist(), c.tag.decode()


def check_rows(logits, greedy, hist, t, tok, edited, phrases, n_valid=0, src_div=1, **rule):
    """the harness' outputs against the rule, bit for bit, as constrain_util.check_rows; returns per logits row whether
    g was in E"""
    logits = np.asarray(logits, f32)
    RS, ld = logits.shape
    nv = n_valid or ld
    hit = []
    for q in range(RS):
        want, wtok, E = apply(logits[q, :nv], hist[q * src_div, :t], phrases, **rule)
        got = edited[q]
        assert (got[:nv].view(np.uint32) == want.view(np.uint32)).all(), \
            f"row {q}: edited logits differ at columns {np.flatnonzero(got[:nv].view(np.uint32) != want.view(np.uint32))[:8]}"
        assert (got[nv:].view(np.uint32) == logits[q, nv:].view(np.uint32)).all(), f"row {q}: a column past n_valid changed"
        out = np.setdiff1d(np.arange(nv), np.fromiter(E, int, len(E)))
        assert (got[out].view(np.uint32) == logits[q, out].view(np.uint32)).all(), f"row {q}: a column outside E changed"
        assert (tok[q * src_div:(q + 1) * src_div] == wtok).all(), f"row {q}: tokens {tok[q * src_div:(q + 1) * src_div]}, the rule's {wtok}"
        hit.append(int(greedy[q]) in E)
    return hit
