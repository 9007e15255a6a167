"""Shared by the decode attention kernel tests (tests/test_gpu_decode_attn_kernels.py and the planted defects of
tests/test_kernel_util_host.py): the ctypes binding of qasr_kt_decode_attention (include/qasr_capi.h,
csrc/kernel_harness.hip), seeded cases poisoned by the cache contract of csrc/kernels.h (above DecodeAttnArgs),
the float64 reference with bounds derived from each kernel's arithmetic (none is measured), the numpy restatement
of the decode chain (fx_decode.h / fx_chain.h) and the comparators.  U = 2^-24.

Cache contract, as the cases poison: K / V rows above pos NaN; row pos +-65504 junk (loaded stale, weight 0);
V^T keys pos + 1 .. 8 (pos / 8) + 7 +-65504 junk (loaded, weight 0), from the next key block on NaN; the rows the
harness appends after the last region NaN.  Mode 4 (chain alone) carries the real V at key pos.
"""
import ctypes as C
import functools

import numpy as np

import attn_util as au
import kernel_util as ku
from attn_util import vt_ctx, vt_index
from kernel_util import GUARD, U, ulp16


class DecodeCall(C.Structure):
    _fields_ = au._i32("mode", "B", "n_head", "n_kv_head", "max_ctx", "max_pos", "grid_splits", "spl1", "spl_batch", "stream_blocks",
                       "kv_nt", "fx_seq", "repeat", "guard") + [("scale", C.c_float), ("eps", C.c_float)] + au._ptr(
        "pos", "qkv", "q_norm", "k_norm", "rope", "scores_in", "kc", "vc", "vt", "scores", "out", "out_b", "out32", "out32_b",
        "outq", "outq_b", "outd", "outd_b") + [("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


PLAIN, SCORES, EXACT, EXACT_SEQ, CHAIN = range(5)
JUNK = 65504.0
LATTICE_SEED, CHAIN_SEED = 2, 1   # picked on the CPU: the restatement's near-tie share stays under 5 % (test_kernel_util_host.py)
HW_EXP2_ULPS = 1.0   # v_exp_f32 behind __expf: 1 ulp in the public CDNA ISA description; MI355X_MICROARCH.md and the CDNA
                     # HIP guide do not state it, so it stays a named constant (measured worst / bound: profiles/decode_attn_tests)


# ==================================================================== cases
def _junk(rng, shape):
    return (rng.integers(0, 2, shape) * 2 - 1).astype(np.float16) * np.float16(JUNK)


@functools.lru_cache(maxsize=None)
def decode_case(pos, n_kv_head, max_ctx, seed, lattice=False, kscale_log2=0, spike=False, wmax=12):
    """one decode step of len(pos) sequences (row b = cache slot b), n_head = 2 n_kv_head, poisoned by the contract.
    lattice: raw q / k entries +-2^e (one e per head, so the RMS norm's scale is exactly 2^-e at eps = 0), norm
    weights multiples of 1/8 up to wmax / 8, rope entries from {(1,0), (0,1), (-1,0), (0,-1), (1/2,1/2)}, cached K multiples of 1/8
    in [-2, 2], scale 2^-3: the normed, rotated fp16 q and k and every fp32 score sum are exact in any order.
    Otherwise real-valued inputs; kscale_log2 scales the cached K and all of V; spike: one cached key per sequence
    scores 40 above the rest for head 0 of every kv group."""
    B, nh, nkv = len(pos), 2 * n_kv_head, n_kv_head
    rng = np.random.default_rng([B, n_kv_head, max_ctx, seed, int(lattice), kscale_log2 + 16, int(spike), wmax])
    max_pos = max_ctx + 5
    W = (nh + 2 * nkv) * 128
    if lattice:
        qkv = (2.0 ** np.repeat(rng.integers(-3, 4, (B, W // 128)), 128, 1) * (rng.integers(0, 2, (B, W)) * 2 - 1)).astype(np.float32)
        qkv[:, (nh + nkv) * 128:] = rng.standard_normal((B, nkv * 128))   # v: any values (one fp16 conversion)
        qn, kn = (rng.integers(-wmax, wmax + 1, (2, 128)) / 8.0).astype(np.float32)
        table = np.array([(1, 0), (0, 1), (-1, 0), (0, -1), (0.5, 0.5)], np.float32)
        rope = table[rng.integers(0, 5, (max_pos, 64))]
        eps, scale = 0.0, 2.0 ** -3
    else:
        qkv = (rng.standard_normal((B, W)) * np.repeat(2.0 ** rng.integers(-3, 4, W // 128), 128)).astype(np.float32)
        qn, kn = (1 + 0.2 * rng.standard_normal((2, 128))).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, (max_pos, 64))
        rope = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
        eps, scale = 1e-6, 128 ** -0.5
    qkv[:, (nh + nkv) * 128:] *= 2.0 ** kscale_log2
    kc = np.full((B, nkv, max_ctx, 128), np.nan, np.float16)
    vc = kc.copy()
    vt = np.full((B, nkv, 128 * vt_ctx(max_ctx)), np.nan, np.float16)
    d = np.arange(128)
    for b, p in enumerate(pos):
        kc[b, :, :p] = (rng.integers(-16, 17, (nkv, p, 128)) / 8.0 if lattice else rng.standard_normal((nkv, p, 128)) * 2.0 ** kscale_log2)
        vc[b, :, :p] = rng.standard_normal((nkv, p, 128)) * 2.0 ** kscale_log2
        kc[b, :, p], vc[b, :, p] = _junk(rng, (nkv, 128)), _junk(rng, (nkv, 128))
        for k in range(p):
            vt[b, :, vt_index(k, d)] = vc[b, :, k].T
        for k in range(p, 8 * (p // 8) + 8):
            vt[b, :, vt_index(k, d)] = _junk(rng, (128, nkv))
    case = dict(B=B, n_head=nh, n_kv_head=nkv, max_ctx=max_ctx, max_pos=max_pos, pos=np.array(pos, np.int32), scale=np.float32(scale),
                eps=eps, qkv=qkv, q_norm=qn, k_norm=kn, rope=rope, kc=kc, vc=vc, vt=vt, lattice=lattice)
    if spike and not lattice:   # cached key p // 2 = alpha q / |q|^2 for head 0 of each group: its score is 40 on top
        q = new_rows(case)[0]
        for b, p in enumerate(pos):
            if p:
                for g in range(nkv):
                    qh = q[b, 2 * g]
                    kc[b, g, p // 2] = (40.0 / scale) * qh / (qh * qh).sum()
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _post_case(case):
    return dict(n_head=case["n_head"], n_kv_head=case["n_kv_head"], rows=case["B"], qkv=case["qkv"], rope=case["rope"],
                row_pos=case["pos"], q_norm=case["q_norm"], k_norm=case["k_norm"], eps=case["eps"])


_ROWS = {}


def new_rows(case):
    """the step's q / k after the norm and the rotation in float64 with their bounds before the fp16 rounding
    (au.qkv_post_ref), and v's exact fp16 rows: (q [B][nh][128], bq, k [B][nkv][128], bk, v fp16 [B][nkv][128])"""
    key = id(case["qkv"])   # (cases are cached and read-only; the rows do not depend on the caches)
    if key not in _ROWS:
        q, bq, k, bk, v = au.qkv_post_ref(_post_case(case))
        B = case["B"]
        _ROWS[key] = (case["qkv"], q.reshape(B, -1, 128), bq.reshape(B, -1, 128), k.reshape(B, -1, 128), bk.reshape(B, -1, 128),
                      v.reshape(B, -1, 128))
    return _ROWS[key][1:]


def new_rows_f32(case):
    """float32 restatement of decode_attn_body's norm and rotation: squares summed in float64, scale = 1 / sqrtf(...),
    two multiplies, the rotation's products and difference each rounded to fp32, one fp16 conversion.  (The device may
    contract the rotation into an fma; for the lattice family every intermediate is exact, so both agree.)"""
    nh, nkv, B = case["n_head"], case["n_kv_head"], case["B"]
    x = case["qkv"].reshape(B, nh + 2 * nkv, 128)[:, :nh + nkv]
    ss = (x * x).astype(np.float64).sum(-1, keepdims=True)
    sc = np.float32(1) / np.sqrt((ss / 128.0).astype(np.float32) + np.float32(case["eps"]), dtype=np.float32)
    w = np.concatenate([np.repeat(case["q_norm"][None], nh, 0), np.repeat(case["k_norm"][None], nkv, 0)])[None]
    y = ((x * sc).astype(np.float32) * w).astype(np.float32)
    cs = case["rope"][case["pos"]]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    y0, y1 = y[..., :64], y[..., 64:]
    r = np.concatenate([(y0 * c).astype(np.float32) - (y1 * s).astype(np.float32), (y0 * s).astype(np.float32) + (y1 * c).astype(np.float32)],
                       -1).astype(np.float32)
    return r[:, :nh].astype(np.float16), r[:, nh:].astype(np.float16)


def _straddle(x, b):
    """one fp16 ulp where [x - b, x + b] holds an fp16 rounding boundary (the kernel's fp32 value lies in it and may
    round to the neighbour), 0 elsewhere"""
    return np.where((x + b).astype(np.float16) != (x - b).astype(np.float16), ulp16(x), 0.0)


def keys_of(case, b, g, stale=False):
    """(K, V) float64 [pos + 1][128] of sequence b, kv group g after the step: the cached rows below pos and the new
    row (fp16 of the float64 reference).  stale: the planted defect -- the cache's own row pos instead"""
    p = int(case["pos"][b])
    _, _, k, _, v = new_rows(case)
    K, V = case["kc"][b, g, :p + 1].astype(np.float64), case["vc"][b, g, :p + 1].astype(np.float64)
    if not stale:
        K[p], V[p] = k[b, g].astype(np.float16).astype(np.float64), v[b, g].astype(np.float64)
    return K, V


# ================================================================ reference
def split_of(case, call):
    """keys per split of the launch (attention.hip decode_split_keys); 0 = the per-sequence kernel"""
    if case["B"] <= 8:
        s1 = call.get("spl1", 0)
        return s1 if s1 in (64, 128) else 128 if call["grid_splits"] >= 30 else 64
    if call.get("stream_blocks", 0) > 0 and case["n_kv_head"] * case["B"] >= call["stream_blocks"] // 2:
        return 0
    return 128 if call.get("spl_batch", 256) == 128 else 256


def decode_reference(case, spl, grid_splits, defect=None):
    """float64 softmax attention of every (sequence, head) with the bound of the split kernels (spl 64 / 128 / 256
    keys a split) or the per-sequence kernel (spl 0), [B][n_head * 128].
      * Scores: fp16 x fp16 products are exact in fp32; 128 MFMA additions and the scale: (128 + 2) U scale sum |q k|.
        The kernel's fp16 q (and the new k) is the rounding of an fp32 value within au.qkv_post_ref's bound of the
        float64 one: the same fp16 value as the reference's unless that interval straddles a rounding boundary, where
        it is the neighbour (_straddle): scale (dq |k| + |q| dk + dq dk).
      * Split kernels: p = expf(s - m_split) (in au.softmax_terms: the subtraction, expf 2 U); the combiner weighs a
        split by __expf(m_split - Mn), exp2 of the argument times fl(log2 e): the constant and the product each round
        once, |x| U each in the exponent, i.e. 2 U (M - m_split) here, and the hardware exp2 HW_EXP2_ULPS ulps,
        2 U each at their largest relative size; every pass of 16 splits rescales by expf(M - Mn): tiles = passes
        (softmax_terms' tiles + 1 covers the weight's own subtraction and multiply).  A term passes spl / 16 fmas in
        its lane, the 16-way LDS sum and one fma per split: adds = spl / 16 + 16 + splits.
      * Per-sequence kernel: every 64-key chunk rescales the wave's (l, O): tiles = chunks; four fmas a chunk in the
        lane, two shuffles, four waves (l: the 6-step wave sum): adds = 4 chunks + 10.
      * 1 / L and the multiply: 3 U |O| (softmax_terms); fp16 outputs half an ulp (the comparator).
    defect: 'stale' | 'drop_last_split' | 'empty_split' | 'seam_twice' | 'next_key' -- one planted defect"""
    B, nh, nkv = case["B"], case["n_head"], case["n_kv_head"]
    q, bq, k, bk, _ = new_rows(case)
    qh = q.astype(np.float16).astype(np.float64)
    dq, dk = _straddle(q, bq), _straddle(k, bk)
    scale = float(case["scale"])
    ref, bound = np.zeros((B, nh * 128)), np.zeros((B, nh * 128))
    for b in range(B):
        p = int(case["pos"][b])
        n = p + 1
        for h in range(nh):
            g = h // 2
            K, V = keys_of(case, b, g, stale=defect == "stale")
            if defect == "next_key":   # key pos + 1 attended: whatever the cache holds there
                K = np.vstack([K, case["kc"][b, g, p + 1:p + 2].astype(np.float64)])
                V = np.vstack([V, case["vc"][b, g, p + 1:p + 2].astype(np.float64)])
            if defect == "drop_last_split" and p >= 64:
                K, V = K[:p // 64 * 64], V[:p // 64 * 64]
            if defect == "seam_twice" and p >= 64:   # key 64, the first of the second split, also taken by the first
                K, V = np.vstack([K, K[64:65]]), np.vstack([V, V[64:65]])
            nk = len(K)
            dK = np.zeros_like(K)
            if defect is None:
                dK[p] = dk[b, g]
            s = scale * (qh[b, h] @ K.T)[None]
            mag = scale * (np.abs(qh[b, h]) @ np.abs(K).T)[None]
            eps = (128 + 2) * U * mag + scale * ((dq[b, h] @ np.abs(K).T) + (np.abs(qh[b, h]) + dq[b, h]) @ dK.T)[None]
            if spl:
                nsp = (grid_splits * 64 + spl - 1) // spl
                msp = np.array([s[0, i:i + spl].max() for i in range(0, nk, spl)])
                eps = eps + (2 * U * np.repeat(s.max() - msp, spl)[:nk])[None] + 2 * HW_EXP2_ULPS * U
                tiles, adds = (nsp + 15) // 16, spl // 16 + 16 + nsp
            else:
                chunks = (n + 63) // 64
                tiles, adds = chunks, 4 * chunks + 10
            o, bd = au.softmax_terms(s, eps, V, np.ones(s.shape, bool), tiles=tiles, adds=adds)
            if defect == "empty_split":   # an empty split joins the denominator with weight 1 (relative to the maximum)
                D = np.exp(s - s.max()).sum()
                o = o * D / (D + 1)
            ref[b, 128 * h:128 * h + 128], bound[b, 128 * h:128 * h + 128] = o[0], bd[0]
    return ref, bound


def lattice_scores(case):
    """the lattice family's scaled scores in float64 (exact, and exactly fp32) [B][nh][max_ctx], NaN past pos, after
    asserting that the float32 restatement of the norm and rotation gives the float64 reference's fp16 q and k bit for
    bit and that the float32 score sums equal the float64 ones"""
    assert case["lattice"]
    B, nh = case["B"], case["n_head"]
    q, bq, k, bk, _ = new_rows(case)
    q16, k16 = new_rows_f32(case)
    assert np.array_equal(q16.astype(np.float64), q) and np.array_equal(k16.astype(np.float64), k), \
        "lattice family: the normed, rotated q / k are not exact fp16 values"
    s = np.full((B, nh, case["max_ctx"]), np.nan)
    for b in range(B):
        p = int(case["pos"][b])
        for h in range(nh):
            K, _ = keys_of(case, b, h // 2)
            dots32 = K.astype(np.float32) @ q16[b, h].astype(np.float32)
            dots = K @ q[b, h]
            assert np.array_equal(dots32.astype(np.float64), dots), "lattice family: fp32 score sums are not exact"
            s[b, h, :p + 1] = (dots32 * np.float32(case["scale"])).astype(np.float64)
    return s


# ==================================================================== chain
def chain_rel(s, chunks):
    """relative bound of the decode chain's S and the divide (fx_weights_reg): a key's vs = expf(s - Mp), 2 U and
    the subtraction; it then rides through the lane's up to 32 sequential S = S ms + vs steps (two roundings each,
    64 U; every ms an expf, 2 U each, their subtractions telescoping to the spread), the lane's rescale to the chunk
    maximum (expf, subtraction, multiply), the 6-step wave sum and per 2048-key chunk S expf(Mold - M) + Sc (expf,
    subtraction, multiply, add); 1 / S and the multiply 3 U.  spread = M - min s over the keys."""
    spread = float((s.max(-1) - s.min(-1)).max())
    return (2 + 64 + 64 + 3 + 6 + 5 * chunks + 3 + (3 + chunks) * spread) * U


def decode_chain(s, V, expf=au._expf, vshift=0, skip_rescale_from=None):
    """numpy restatement of ggml's chain as fx_decode.h runs it for one sequence: s fp32 [heads][n] scaled scores,
    V float64 [heads][n][128] (fp16 values), keys in order: a new maximum rescales, acc = fp16(fp32(acc) ms), ms =
    expf(M - s) (0 at the first key), and takes vs = 1; any other key vs = expf(s - M); every key acc =
    fp16(fma(v, vs, acc)).  Near-tie marks as au.exact_chain.  Returns (acc / S in float64 [heads][128], marks, one
    fp16 ulp of the largest prefix |acc| over S).
    Planted defects: vshift -- V of key k taken from key k + vshift (a wrong V^T block is vshift = 8);
    skip_rescale_from -- no rescale of the accumulator at a new maximum from that key on"""
    H, n = s.shape
    s = s.astype(np.float32)
    M = np.full(H, -np.inf, np.float32)
    acc, peak, tied = np.zeros((H, 128)), np.zeros((H, 128)), np.zeros((H, 128), bool)
    for j in range(n):
        sj = s[:, j]
        new = sj > M
        with np.errstate(invalid="ignore", over="ignore"):
            vs = np.where(new, np.float32(1), expf(np.where(new, np.float32(0), sj - M))).astype(np.float64)
            if new.any() and (skip_rescale_from is None or j < skip_rescale_from):
                hi = np.nonzero(new)[0]
                ms = np.where(np.isneginf(M[hi]), np.float32(0), expf(M[hi] - sj[hi])).astype(np.float64)
                un = acc[hi] * ms[:, None]
                tied[hi] |= au._near16(un, 2.0 ** -22 * np.abs(un))
                acc[hi] = un.astype(np.float32).astype(np.float16)
        t = V[:, min(j + vshift, n - 1)] * vs[:, None]
        un = t + acc
        tied |= au._near16(un, 2.0 ** -22 * np.abs(t)) & ~new[:, None]
        acc = un.astype(np.float32).astype(np.float16).astype(np.float64)
        np.maximum(peak, np.abs(acc), out=peak)
        M = np.maximum(M, sj)
    S = np.exp(s.astype(np.float64) - M.astype(np.float64)[:, None]).sum(1)
    return acc / S[:, None], tied, ulp16(peak) / S[:, None]


def chain_reference(scores, vals, pos, **defect):
    """decode_chain over a batch: scores [B][nh][>= pos + 1] (fp32-exact), vals(b, h) -> V float64 [pos + 1][128].
    Returns (ref, marks, amax, rel) as [B][nh * 128] ([B][1] for rel)"""
    B, nh = scores.shape[:2]
    ref, tie, amax, rel = np.zeros((B, nh * 128)), np.zeros((B, nh * 128), bool), np.zeros((B, nh * 128)), np.zeros((B, 1))
    for b in range(B):
        n = int(pos[b]) + 1
        s = scores[b, :, :n]
        V = np.stack([vals(b, h) for h in range(nh)])
        o, t, a = decode_chain(s, V, **defect)
        ref[b], tie[b], amax[b] = o.reshape(-1), t.reshape(-1), a.reshape(-1)
        rel[b] = chain_rel(s.astype(np.float64), (n + 2047) // 2048)
    return ref, tie, amax, rel


def lattice_chain(case, **defect):
    """the chain reference of a lattice case's own scores (modes 2 and 3)"""
    return chain_reference(lattice_scores(case), lambda b, h: keys_of(case, b, h // 2)[1], case["pos"], **defect)


def chain_bound(chain):
    ref, tie, amax, rel = chain
    return np.abs(ref) * rel + np.where(tie, 2 * amax, 0.0)


def check_chain(buf, chain, fp16, what):
    """an exact launch's output against the restatement: unmarked elements within the relative bound of S and the
    divide (their accumulators equal to the last bit), marked ones additionally within 2 fp16 ulps of the largest
    prefix accumulator over S.  Returns (worst error / bound, marked share); the share is capped at 5 %"""
    ref, tie = chain[0], chain[1]
    share = float(tie.mean())
    assert share <= 0.05, f"{what}: {share:.3f} of the elements are near-ties -- the case no longer holds the chain to its bits"
    out = ku.in_range(buf, ref.shape[0], ref.shape[1], what)
    return ku.check_values(out, ref, chain_bound(chain), fp16=fp16, what=what), share


@functools.lru_cache(maxsize=None)
def chain_case(pos, ratio, n_kv_head, max_ctx, seed, rise=None, sigma=2.0):
    """mode 4: scores the caller supplies (normal, deviation sigma) and a full V^T cache (real V through key pos, junk to
    the end of pos's block, NaN after).  rise: 'late' puts the largest score at key 2048 of the sequences that have
    it (the maximum rises in the second weights chunk), 'early' at key 5 (it never rises there)"""
    B, nh = len(pos), ratio * n_kv_head
    rng = np.random.default_rng([B, ratio, n_kv_head, max_ctx, seed, int(8 * sigma)])
    scores = np.full((B, nh, max_ctx), np.nan, np.float32)
    V = np.full((B, n_kv_head, max_ctx, 128), np.nan, np.float16)
    vt = np.full((B, n_kv_head, 128 * vt_ctx(max_ctx)), np.nan, np.float16)
    d = np.arange(128)
    for b, p in enumerate(pos):
        scores[b, :, :p + 1] = sigma * rng.standard_normal((nh, p + 1))
        if rise and p >= 2048:
            scores[b, :, 2048 if rise == "late" else 5] = 4.5 * sigma
        V[b, :, :p + 1] = rng.standard_normal((n_kv_head, p + 1, 128))
        for k in range(p + 1):
            vt[b, :, vt_index(k, d)] = V[b, :, k].T
        for k in range(p + 1, 8 * (p // 8) + 8):
            vt[b, :, vt_index(k, d)] = _junk(rng, (128, n_kv_head))
    case = dict(B=B, n_head=nh, n_kv_head=n_kv_head, max_ctx=max_ctx, max_pos=max_ctx, pos=np.array(pos, np.int32), scale=np.float32(1),
                eps=0.0, scores_in=scores, vt=vt, V=V, ratio=ratio)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def chain_case_reference(case, **defect):
    return chain_reference(case["scores_in"], lambda b, h: case["V"][b, h // case["ratio"], :case["pos"][b] + 1].astype(np.float64),
                           case["pos"], **defect)


# ================================================================== running
def run_decode(case, mode, kind="f32", *, grid_splits=None, repeat=1, expect_rc=0, **call):
    """kind: 'f32' | 'f16' | 'q8' (mode SCORES: the scores instead).  Returns an Out with tag and the whole allocations:
    out / out32 / outq + outd (and *_b with repeat 2), scores, kc, vc, vt"""
    B, nh = case["B"], call.pop("n_head", case["n_head"])   # (overrides, for the declines: never more heads than the case holds)
    if grid_splits is None:
        grid_splits = int(case["pos"].max()) // 64 + 1
    c = DecodeCall(mode=mode, B=B, n_head=nh, n_kv_head=call.pop("n_kv_head", case["n_kv_head"]),
                   max_ctx=call.pop("max_ctx", case["max_ctx"]), max_pos=case["max_pos"], grid_splits=grid_splits, repeat=repeat,
                   guard=GUARD, scale=float(case["scale"]), eps=case["eps"], spl1=call.pop("spl1", 0), spl_batch=call.pop("spl_batch", 256),
                   stream_blocks=call.pop("stream_blocks", 0), kv_nt=call.pop("kv_nt", 1), fx_seq=call.pop("fx_seq", 1))
    assert not call, call
    QD = nh * 128
    outs = {}
    for sfx in ("", "_b")[:repeat]:
        if mode == SCORES:
            continue
        if kind == "q8":
            outs.update({"outq" + sfx: au._out(B, QD, np.int8), "outd" + sfx: au._out(B, QD // 32, np.float32)})
        else:
            outs.update({("out32" if kind == "f32" else "out") + sfx: au._out(B, QD, np.float32 if kind == "f32" else np.uint16)})
    if mode == SCORES:
        outs["scores"] = au._out(B * nh, case["max_ctx"], np.float32)
    outs["vt"] = ku.bits(case["vt"]).copy()
    ins = {}
    if mode == CHAIN:
        ins["scores_in"] = case["scores_in"]
    else:
        outs.update(kc=ku.bits(case["kc"]).copy(), vc=ku.bits(case["vc"]).copy())
        ins = {k: case[k] for k in ("qkv", "q_norm", "k_norm", "rope")}
    keep = ku._set(c, [], pos=case["pos"], **ins, **outs)
    if au._call("qasr_kt_decode_attention", c, keep, expect_rc):
        return None
    r = au.Out(c, outs)
    r.tag = c.tag.decode()
    return r


def check_caches(r, case, what):
    """K / V / V^T equal the input except row / column pos: K within au.qkv_post_ref's bound, V one fp16 conversion
    bit for bit, V^T the same values through vt_index.  Returns K's worst error / bound"""
    B, nkv = case["B"], case["n_kv_head"]
    _, _, k, bk, v = new_rows(case)
    pos = case["pos"]
    bi = np.arange(B)
    wk, wv, wt = ku.bits(case["kc"]).copy(), ku.bits(case["vc"]).copy(), ku.bits(case["vt"]).copy()
    gk = r.kc.reshape(wk.shape)
    newk = gk[bi, :, pos].copy()
    wk[bi, :, pos] = newk
    assert np.array_equal(gk, wk), f"{what}: a K cache row other than pos changed"
    wv[bi, :, pos] = v.view(np.uint16)
    assert np.array_equal(r.vc.reshape(wv.shape), wv), f"{what}: the V cache is not the input with fp16(v) at row pos"
    d = np.arange(128)
    for b in range(B):
        wt[b, :, vt_index(int(pos[b]), d)] = v[b].view(np.uint16).T
    assert np.array_equal(r.vt.reshape(wt.shape), wt), f"{what}: the V^T cache is not the input with fp16(v) at column pos"
    return ku.check_values(newk.reshape(B, -1), k.reshape(B, -1), bk.reshape(B, -1), fp16=True, what=what + " K row")


def fake(vals, fp16=False):
    """the allocation a kernel computing vals [B][QD] would leave"""
    return au.fake_output(vals, np.ones(len(vals), bool), fp16)
