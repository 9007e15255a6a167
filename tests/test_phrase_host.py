"""CPU: hotword boosting without a device -- hand-made known answers of the rule's numpy restatement
(tests/phrase_util.py), the phrase compiler (csrc/phrase_host.h, through tools/phrase_host_check.cpp,
once more under the host sanitizers) against the brute-force rule, qasr_phrases_validate on every range edge,
qasr_phrase_tokenize on a host-only model and the CLI's flag errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import phrase_util as pu
import qasr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
QASR_ERR_ARG = 1
NAMES = ("qasr_phrases_validate", "qasr_set_phrases", "qasr_get_phrases", "qasr_phrase_tokenize", "qasr_kt_phrases")


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ------------------------------------------------------------------ the rule
def test_position_zero_always_matches_and_a_short_history_does_not():
    ph = [([7, 8, 9], 2.0)]
    assert pu.bonuses(ph, []) == ({7: f32(2.0)}, 0)
    assert pu.bonuses(ph, [1, 2, 3]) == ({7: f32(2.0)}, 0)
    assert pu.bonuses(ph, [7]) == ({7: f32(2.0), 8: f32(2.0)}, 1)
    assert pu.bonuses(ph, [7, 8]) == ({7: f32(2.0), 9: f32(2.0)}, 2)
    # t < j: a history of one token cannot match position 2, whatever it holds
    assert pu.bonuses(ph, [8])[0] == {7: f32(2.0)}
    assert pu.bonuses(ph, [7, 8, 9])[0] == {7: f32(2.0)}           # the phrase is complete: only its start again
    assert pu.bonuses(ph, [8, 7])[0] == {7: f32(2.0), 8: f32(2.0)}


def test_the_maximum_decides_not_the_deepest_match():
    a, b, c = 1, 2, 3
    ph = [([a, b, c], 1.0), ([b, c], 8.0)]
    bon, deep = pu.bonuses(ph, [a, b])
    assert bon == {c: f32(8.0), a: f32(1.0), b: f32(8.0)} and deep == 2
    l = np.zeros(6, f32)
    out, tok, E = pu.apply(l, [a, b], ph)
    assert out.tolist() == [0, 1, 8, 8, 0, 0] and tok == b and E == {a, b, c}
    # the other way round: the deeper phrase holds the larger boost
    assert pu.bonuses([([a, b, c], 8.0), ([b, c], 1.0)], [a, b])[0][c] == f32(8.0)


def test_duplicates_single_tokens_and_the_longest_phrase():
    assert pu.bonuses([([4, 5], 1.0), ([4, 5], 3.0), ([4, 5], 2.0)], [4])[0] == {4: f32(3.0), 5: f32(3.0)}
    assert pu.bonuses([([9], 0.5)], [9, 9, 9]) == ({9: f32(0.5)}, 0)
    long = list(range(20, 36))
    bon, deep = pu.bonuses([(long, 4.0)], [3] + long[:15])
    assert deep == 15 and bon == {20: f32(4.0), 35: f32(4.0)}
    assert pu.bonuses([(long, 4.0)], long[:15])[1] == 15 and pu.bonuses([(long, 4.0)], long[1:15])[1] == 0


def test_the_boost_step_sits_between_the_bias_and_the_ban():
    l = np.array([1.0, 5.0, 2.0, 0.5, -3.0], f32)
    ph = [([1, 2], 4.0), ([3], 0.25)]
    # penalty, bias, boost on one column, each one rounded operation in that order: ((5 / 2) + 1) + 4
    out, tok, E = pu.apply(l, [1], ph, p=2.0, bias={1: 1.0})
    assert out[1] == f32(7.5) and out[2] == f32(6.0) and out[3] == f32(0.75) and tok == 1 and E == {1, 2, 3}
    # a banned column stays -inf whatever its boost, and the token avoids it
    out, tok, E = pu.apply(l, [1], ph, n=1)
    assert out[1] == -np.inf and out[2] == f32(6.0) and tok == 2
    # two adds, not one add of the sum: (2^24 + 1) + 1 in fp32 stays 2^24
    l2 = np.array([2.0 ** 24, 0.0], f32)
    out, _, _ = pu.apply(l2, [], [([0], 1.0)], bias={0: 1.0})
    assert bits(out[0]) == bits(f32(2.0 ** 24)) and f32(2.0 ** 24) + f32(2.0) != f32(2.0 ** 24)
    # no phrases: constrain_util's rule
    import constrain_util as cu
    a, b = pu.apply(l, [1, 3, 1], None, n=2, p=1.3, bias={0: 0.5}), cu.apply(l, [1, 3, 1], n=2, p=1.3, bias={0: 0.5})
    assert (bits(a[0]) == bits(b[0])).all() and a[1:] == b[1:]


# ------------------------------------------------- the compiler against the rule
def _hex(x):
    return f"{int(np.float32(x).view(np.uint32)):08x}"


def _case(phrases, hists, vocab):
    ph = pu.split(phrases)
    lines = [f"{len(ph)} {vocab} {len(hists)}"]
    lines += [f"{len(ids)} {_hex(b)} " + " ".join(map(str, ids)) for ids, b in ph]
    lines += [f"{len(h)} " + " ".join(map(str, h)) for h in hists]
    return "\n".join(lines) + "\n"


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "qwen3-asr.cpp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "phrase_host_check.cpp"), "-o", exe], check=True)
    return exe


def _random_cases(n_cases=220, seed=31):
    """lists over 12 tokens (prefixes, suffixes and duplicates collide), lengths 1..16, coarse boosts (ties), and
    histories of length 0..40 partly spelled from the phrases themselves (deep matches)"""
    rng = np.random.default_rng(seed)
    cases = []
    for ci in range(n_cases):
        n_ph = int(rng.integers(1, 30))
        V = 12 if ci % 4 else 3
        phrases = []
        for _ in range(n_ph):
            ln = int(rng.integers(1, 17))
            ids = rng.integers(0, V, ln).tolist()
            if phrases and rng.random() < 0.3:      # an extension, a suffix or a copy of an earlier one
                base = phrases[int(rng.integers(len(phrases)))][0]
                kind = rng.integers(3)
                ids = (base + ids)[:16] if kind == 0 else base[int(rng.integers(len(base))):] if kind == 1 else list(base)
            phrases.append((ids, float(rng.integers(1, 9)) / 2))
        hists = []
        for hi in range(6):
            t = int(rng.integers(0, 41)) if hi else 0
            h = rng.integers(0, V, t).tolist()
            if t and rng.random() < 0.7:            # end in the beginning of a phrase
                ids = phrases[int(rng.integers(n_ph))][0]
                k = int(rng.integers(1, min(len(ids), t) + 1))
                h[t - k:] = ids[:k]
            hists.append(h)
        cases.append((phrases, hists, V))
    return cases


def _check_output(out, cases):
    at, deep = 0, 0
    for ci, (phrases, hists, _) in enumerate(cases):
        assert out[at].startswith("case ok "), (ci, out[at])
        nodes, edges = map(int, out[at].split()[2:])
        assert edges == nodes - 1 and nodes - 1 == len({tuple(ids[:k]) for ids, _ in phrases for k in range(1, len(ids) + 1)})
        for hi, h in enumerate(hists):
            want, d = pu.bonuses(phrases, h)
            deep = max(deep, d)
            head, _, pairs = out[at + 1 + hi].partition("|")
            got = {int(a): int(b, 16) for a, b in (x.split(":") for x in pairs.split())}
            assert head.split() == ["hist", str(len(want))], (ci, hi)
            assert got == {x: int(bits(b)) for x, b in want.items()}, (ci, hi, phrases, h)
        at += 1 + len(hists)
    assert at == len(out)
    return deep


def test_compiler_equals_the_brute_force_rule(built, tmp_path):
    exe = _build(tmp_path, "phrase_host_check")
    cases = _random_cases()
    assert len(cases) >= 200
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case(*c) for c in cases))
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert _check_output(out, cases) == 15          # some history spelled 15 tokens of a 16-token phrase


def _limit_cases():
    """4096 phrases that share the root's 64 children (57,408 edges); 4096 disjoint phrases of 16 tokens: exactly
    65,536 edges, the most a list inside its ranges can ask for"""
    full = [([k // 64, 64 + k % 64] + [200 + k] * 13, 1.0) for k in range(4096)]
    exact = [([1000 + k] + [k] * 15, 2.0) for k in range(4096)]
    return full, exact


def test_compiler_limits(built, tmp_path):
    exe = _build(tmp_path, "phrase_host_check")
    full, exact = _limit_cases()
    text = _case(full, [[0, 64, 200]], 0) + _case(exact, [[1000, 0, 0]], 0) + _case(exact + [([9], 1.0)], [], 0)
    path = tmp_path / "limits.txt"
    path.write_text(text)
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "case ok 57409 57408" and out[1] == f"hist 65 |" + "".join(f" {k}:{_hex(1.0)}" for k in range(64)) + f" 200:{_hex(1.0)}"
    assert out[2] == "case ok 65537 65536" and out[3] == f"hist 4097 | 0:{_hex(2.0)}" + "".join(f" {k}:{_hex(2.0)}" for k in range(1000, 5096))
    assert out[4] == "case err phrases: n_phrases must be in 0..4096" and len(out) == 5
    # a 65,537th edge: no list inside the ranges reaches it (4096 x 16 = 65,536), so the compiler is handed one past
    # them (--no-ranges: the last phrase 17 tokens long); the same list inside the ranges is accepted above
    over = exact[:-1] + [(exact[-1][0] + [7], 2.0)]
    path.write_text(_case(over, [], 0))
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["case err phrases: the length of phrase 4095 must be in 1..16"]
    out = subprocess.run([exe, str(path), "--no-ranges"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["case err phrases: the trie exceeds 65536 edges (65537 nodes)"]


def test_compiler_under_the_host_sanitizers(built, tmp_path):
    """the same program and cases with -fsanitize=address,undefined (a stand-alone program: no preload needed)"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    exe = _build(tmp_path, "phrase_host_check_san", san)
    cases = _random_cases(n_cases=60, seed=32)
    full, exact = _limit_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case(*c) for c in cases) + _case(exact, [[1000] + [0] * 14], 0) + _case(exact + [([9], 1.0)], [], 0))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    _check_output(out[:-3], cases)
    assert out[-3] == "case ok 65537 65536" and out[-2].startswith("hist 4097 | 0:") and out[-1].startswith("case err ")


# ------------------------------------------------------------------ the C ABI
def raw(phrases):
    n, ids, ln, val = pu.flat(phrases)
    p = qasr.Phrases(n, ids.ctypes.data_as(C.POINTER(C.c_int32)), ln.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float)))
    return p, (ids, ln, val)


def validate(phrases, vocab=100):
    p, _keep = raw(phrases)
    rc = qasr.lib().qasr_phrases_validate(C.byref(p), vocab)
    return rc, qasr.lib().qasr_last_error().decode()


def test_validate_every_range_edge(built):
    ok = lambda ph, **kw: validate(ph, **kw)[0] == 0
    def bad(word, ph, **kw):
        rc, msg = validate(ph, **kw)
        return rc == QASR_ERR_ARG and word in msg
    assert ok([]) and ok([[0]]) and ok([[99] * 16]) and ok([([5], 100.0)]) and ok([([5], 1e-30)])
    assert ok([[1, 2], [1, 2], [1], [2, 1, 2]])                            # duplicates, prefixes, suffixes
    assert bad("1..16", [[1] * 17]) and bad("outside the vocabulary", [[100]]) and bad("outside the vocabulary", [[3, -1]])
    assert ok([[10 ** 6]], vocab=0)                                        # vocab <= 0: no upper bound
    for b in (0.0, -1.0, 100.00001, float("nan"), float("inf"), float("-inf")):
        assert bad("(0, 100]", [([5], b)]), b
    assert ok([[k % 100] for k in range(4096)]) and bad("0..4096", [[k % 100] for k in range(4097)])
    p, _keep = raw([[1, 2]])
    lib = qasr.lib()
    p.len[0] = 0
    assert lib.qasr_phrases_validate(C.byref(p), 0) == QASR_ERR_ARG and "1..16" in lib.qasr_last_error().decode()
    p.len[0] = 2
    p.n_phrases = -1
    assert lib.qasr_phrases_validate(C.byref(p), 0) == QASR_ERR_ARG and "0..4096" in lib.qasr_last_error().decode()
    for null in ("ids", "len", "boost"):
        q, _k = raw([[1, 2]])
        setattr(q, null, None)
        assert lib.qasr_phrases_validate(C.byref(q), 0) == QASR_ERR_ARG and "without ids, len and boost" in lib.qasr_last_error().decode()
    assert lib.qasr_phrases_validate(None, 0) == QASR_ERR_ARG
    # the Python helper raises with the message
    qasr.phrases_validate([[1, 2], ([3], 7.5)], vocab=100)
    with pytest.raises(qasr.QasrError, match="1..16"):
        qasr.phrases_validate([[1] * 17])
    with pytest.raises(qasr.QasrError, match="tokenizer"):
        qasr.phrases_validate(["text"])
    p, keep = qasr.make_phrases([[1, 2], ([3], 7.5), (4, 5)], boost=2.0)
    assert p.n_phrases == 3 and keep[0].tolist() == [1, 2, 3, 4, 5] and keep[1].tolist() == [2, 1, 2] and keep[2].tolist() == [2.0, 7.5, 2.0]


def test_capi_declares_and_exports_phrases(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and hasattr(lib, n), n
    assert set(NAMES[:4]) <= set(qasr.EXPORTS) and NAMES[4] not in qasr.EXPORTS
    assert "#define QASR_PHRASE_MAX 4096" in hdr and "#define QASR_PHRASE_LEN_MAX 16" in hdr
    assert (qasr.QASR_PHRASE_MAX, qasr.QASR_PHRASE_LEN_MAX) == (4096, 16) == (pu.PHRASE_MAX, pu.PHRASE_LEN_MAX)
    assert C.sizeof(qasr.Phrases) == 32 and C.sizeof(qasr.Constraints) == 32
    # the harness struct: qasr_kt_constrain_args' fields first, at the same offsets
    import constrain_util as cu
    for name, _ in cu.ConstrainCall._fields_[:23]:
        assert getattr(pu.PhraseCall, name).offset == getattr(cu.ConstrainCall, name).offset, name
    lib.qasr_kt_phrases.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_phrases.restype = C.c_int
    assert lib.qasr_kt_phrases(0, None) == QASR_ERR_ARG
    assert lib.qasr_set_phrases(None, None) == QASR_ERR_ARG
    assert lib.qasr_get_phrases(None, None, None, None, None, 0, 0) == QASR_ERR_ARG
    assert lib.qasr_phrase_tokenize(None, b"x", None, None, 0) == -QASR_ERR_ARG


# ------------------------------------------------------------- tokenisation
SPACE = 220      # the synthetic vocabulary's symbol of the byte 0x20


def test_phrase_tokenize_on_a_host_only_model(tiny_gguf, tmp_path):
    m = qasr.Model(tiny_gguf, qasr.QASR_HOST_ONLY if hasattr(qasr, "QASR_HOST_ONLY") else -1)
    try:
        ab = m.tokenize("ab")
        assert m.phrase_tokenize("ab") == [ab, [SPACE] + ab]                       # the leading space changes the ids
        assert m.phrase_tokenize("  ab cd \n") == [m.tokenize("ab cd"), [SPACE] + m.tokenize("ab cd")]      # trimmed
        assert m.detokenize(m.phrase_tokenize("Hi there")[1]) == " Hi there"
        for empty in ("", "   ", "\t\n"):
            with pytest.raises(qasr.QasrError, match="empty"):
                m.phrase_tokenize(empty)
        assert len(m.tokenize("a b c d e f g h")) == 15
        assert [len(v) for v in m.phrase_tokenize("a b c d e f g h")] == [15, 16]
        with pytest.raises(qasr.QasrError, match="1..16"):
            m.phrase_tokenize("a b c d e f g h i")                                 # 17 tokens
        with pytest.raises(qasr.QasrError, match="1..16"):
            m.phrase_tokenize("a b c d e f g h!")                                  # 16 tokens, 17 with the leading space
        assert len(m.tokenize("a b c d e f g h!")) == 16
        lib = qasr.lib()
        ids, ln = (C.c_int32 * 32)(), (C.c_int32 * 2)()
        assert lib.qasr_phrase_tokenize(m.h, b"ab", ids, ln, 2) == -QASR_ERR_ARG and "fewer entries" in lib.qasr_last_error().decode()
        assert lib.qasr_phrase_tokenize(m.h, b"ab", ids, ln, 3) == 2 and list(ln) == [1, 2] and list(ids[:3]) == ab + [SPACE] + ab
    finally:
        m.close()
    # a vocabulary without a symbol for the space byte: both tokenisations are the same ids, one variant
    data = bytearray(open(tiny_gguf, "rb").read())
    sym = "Ġ".encode()
    entry = (2).to_bytes(8, "little") + sym
    at = data.find(entry)
    assert at > 0 and data.find(entry, at + 1) < 0
    data[at + 8:at + 10] = b"~~"
    path = str(tmp_path / "no-space.gguf")
    open(path, "wb").write(data)
    m = qasr.Model(path, -1)
    try:
        assert m.phrase_tokenize("ab") == [m.tokenize("ab")] and m.phrase_tokenize(" ab cd ") == [m.tokenize("ab cd")]
    finally:
        m.close()


# ------------------------------------------------------------------ the CLI
def test_cli_hotword_flag_errors(built, tmp_path):
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    good = tmp_path / "words.txt"
    good.write_text("# names\nab cd\nHi\t7.5\n\n")
    cases = [(["--hotword"], "requires an argument"), (["--hotword", "  "], "--hotword takes a non-empty text"),
             (["--hotword-boost", "0"], "--hotword-boost takes 0 < b <= 100"), (["--hotword-boost", "101"], "--hotword-boost takes 0 < b <= 100"),
             (["--hotword-boost", "x"], "--hotword-boost takes 0 < b <= 100"), (["--hotword-boost", "nan"], "--hotword-boost takes 0 < b <= 100"),
             (["--hotwords-file", str(tmp_path / "missing.txt")], "cannot read hotwords file")]
    for i, (body, msg) in enumerate((("ab\t0\n", "line 1: the boost after the tab"), ("ab\nHi\tseven\n", "line 2: the boost after the tab"),
                                     ("# c\n\tab\n", "line 2: the boost after the tab"), ("ab\t\n", "line 1: the boost after the tab"),
                                     ("\t3\n", "line 1: no text before the boost"))):
        f = tmp_path / f"bad{i}.txt"
        f.write_text(body)
        cases.append((["--hotwords-file", str(f)], msg))
    for flags, msg in cases:
        r = subprocess.run([cli, "-m", "none.gguf", "-f", "none.wav"] + flags, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (flags, r.stderr)
    # a well-formed file and flags pass the parser: the failure is the missing model
    r = subprocess.run([cli, "-m", str(tmp_path / "none.gguf"), "-f", "none.wav", "--hotwords-file", str(good), "--hotword", "ab", "--hotword-boost", "100"],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode != 0 and "Failed to load model" in r.stderr, r.stderr
    assert "--hotword <text>" in subprocess.run([cli, "--help"], capture_output=True, text=True, env=env, timeout=60).stderr
