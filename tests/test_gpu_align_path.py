"""The monotone path through the engine on the synthetic aligner-tiny model: Context.align_path
against the rule applied to the logits the pass left behind, and the JSON documents with option align_monotone."""
import numpy as np
import pytest

import align_path_util as au
import qasr

pytestmark = pytest.mark.gpu
SR = 16000
TEXTS = ["ab cd ef", "ab cd ef gh ij kl mn op qr st", "xy"]


@pytest.fixture(scope="module")
def al(gpu, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("alp") / "aligner-tiny.gguf")
    qasr.write_synthetic_gguf(p, "aligner-tiny", 42, 1)
    m = qasr.Model(p)
    c = qasr.Context(m, max_batch=3, max_ctx=2048)
    clips = [qasr.synth_pcm(8700 + i, int(s * SR)) for i, s in enumerate((2.0, 6.4, 0.9))]
    yield m, c, clips
    c.close()
    m.close()


def test_align_path_equals_the_rule_on_its_own_logits(al):
    m, c, clips = al
    ids = [m.align_tokenize(t)[0] for t in TEXTS]
    res = c.align_path(clips, ids)
    N = m.hp.classify_num
    z = c.align_logits(sum(len(r[0]) for r in res))
    row = 0
    for pcm, text, (cls, lp, score) in zip(clips, TEXTS, res):
        Cn = min(N, len(pcm) // (16 * 80) + 2)
        NT = 2 * len(text.split())
        assert len(cls) == NT and (np.diff(cls) >= 0).all() and 0 <= min(cls) and max(cls) < Cn
        want, wscore = au.rule(z[row:row + NT], Cn)
        assert cls == want.tolist() and np.float32(score).view(np.uint32) == wscore.view(np.uint32)
        ref = np.asarray(z[row:row + NT], np.float64)[np.arange(NT), want] - au.lse64(z[row:row + NT], N)
        assert np.abs(lp - ref).max() <= 1e-4   # (the kernel test holds the bound; here: the right rows and columns)
        row += NT
    for b in (0, 2):   # alone: the same classes, log-probabilities and score as in the batch
        one = c.align_path([clips[b]], [ids[b]])[0]
        assert one[0] == res[b][0] and one[1].tobytes() == res[b][1].tobytes() and one[2] == res[b][2]
    assert all(u >= 0 for u in c.align_path_last_us())


def test_align_json_monotone_and_the_default_document_unchanged(al):
    m, c, clips = al
    before = c.align_json(clips[1], TEXTS[1])[0]
    assert c.get_option("align_monotone") == 0 and "start_logprob" not in before["words"][0]
    doc = c.align_json(clips[1], TEXTS[1], monotone=True)[0]
    (cls, lp, _), = c.align_path([clips[1]], [m.align_tokenize(TEXTS[1])[0]])
    times = []
    for i, w in enumerate(doc["words"]):
        assert w["start_logprob"] == pytest.approx(float(lp[2 * i]), abs=1e-4) and w["end_logprob"] <= 0.0
        assert w["start"] == pytest.approx(min(cls[2 * i] * 0.08, len(clips[1]) / SR), abs=5e-4)
        times += [w["start"], w["end"]]
    assert [w["word"] for w in doc["words"]] == TEXTS[1].split() and times == sorted(times)
    c.set_option("align_monotone", 1)
    docs = c.align_json_batch(clips, TEXTS)[0]
    c.set_option("align_monotone", 0)
    assert docs[1] == doc and all("end_logprob" in w for d in docs for w in d["words"])
    assert c.get_option("align_monotone") == 0
    assert c.align_json(clips[1], TEXTS[1])[0] == before
