"""Summarise a QASR_DEV_TRACE dump: per-block 100 MHz timestamps of one decode
layer's kernels (QKV GEMV, attention, o-proj, gate/up, down).  Dev tool only."""
import sys

import numpy as np

NAMES = ["qkv_gemv", "attention", "oproj_gemv", "gateup_gemv", "down_gemv"]


def main(path, interleaved=False):
    """interleaved: the QKV role's blocks numbered by kv group (32 q, 16 k, 16 v
    blocks a group: builds before the q-rows-first order) instead of 256 q-row,
    128 k-row, 128 v-row blocks"""
    t = np.fromfile(path, dtype=np.uint64).reshape(6, 4096, 8).astype(np.int64)
    raw0, raw1 = t[0].copy(), t[1].copy()
    # chain workgroups.  Pipelined role (one workgroup a query head): rows 4000 + c = [start, chain start,
    # first chunk published, last chunk published, chain done, published, S done, producer polls], 4040 + c =
    # shader clock at chain start / end, keys, new-maximum keys, slow groups, 4080 + c = the two chain waves'
    # ends and cycles.  Before it (one workgroup a kv group): rows 4000 + g, clocks at 4010 + g
    wide = (t[1][4040:4072, 0] > 0).any()
    ch = t[1][4000:4040] if wide else t[1][4000:4008]
    ch = ch[ch[:, 0] > 0]
    ck = (t[1][4040:4072] if wide else t[1][4010:4018]).copy()
    wv = t[1][4080:4096].copy()
    t[1][4000:4096] = 0
    live = [t[k][t[k][:, 0] > 0] for k in range(5)]
    t0 = min(int(x[:, 0].min()) for x in live if len(x))
    us = lambda v: (v - t0) / 100.0
    prev_end = None
    for k, x in enumerate(live):
        if not len(x):
            continue
        st = x[:, 0]
        if k == 1 and len(ch):   # fused exact attention: split blocks (scores) + chain workgroups
            print(f"{NAMES[k]:12s} split blocks {len(x):4d} start {us(st.min()):7.2f}..{us(st.max()):7.2f}  "
                  f"scores published max {us(x[:, 3].max()):7.2f}")
            if wide:
                lab = ["start", "chain start", "first chunk", "last chunk", "chain", "published", "S done"]
                nl = 7
            else:
                lab = ["start", "v ready", "scores gathered", "weights", "chain", "published", "w expf", "w stored"]
                nl = 8 if (ch[:, 6] > 0).all() else 6
            print(f"{'':12s} chain wgs {len(ch)}: " + "  ".join(f"{lab[i]} {us(np.median(ch[:, i])):6.2f}/{us(ch[:, i].max()):6.2f}"
                                                             for i in range(nl)))
            e = ch[:, 5].max()
            ok = ck[:, 1] > ck[:, 0]
            if ok.any() and len(ch) == len(ck[ok]):
                cyc = (ck[ok, 1] - ck[ok, 0]).astype(np.float64)
                dt = (ch[:, 4] - ch[:, 1]).astype(np.float64) / 100.0   # us, 'v ready' -> 'chain'
                print(f"{'':12s} chain: {np.median(cyc):.0f} shader cycles over {ck[ok, 2][0]} keys "
                      f"({np.median(cyc) / ck[ok, 2][0]:.1f} a key), {np.median(dt):.2f} us -> {np.median(cyc / dt) / 1e3:.2f} GHz; "
                      f"{'per head' if wide else 'head 2g'} new-maximum keys {ck[ok, 3].tolist()}, slow 8-key groups {ck[ok, 4].tolist()}")
                if wide:
                    w2 = wv[wv[:, 0] > 0][:, 2:4].astype(np.float64) / ck[ok, 2][0]
                    print(f"{'':12s} cycles a key per chain wave: median {np.median(w2):.2f}, min {w2.min():.2f}, max {w2.max():.2f}; "
                          f"producer 0 polls a workgroup: median {np.median(ch[:, 7]):.0f}")
        elif k == 1:
            kv, rdy, cnt = x[:, 1], x[:, 2], x[:, 3]
            lastb = x[x[:, 4] > 0]
            print(f"{NAMES[k]:12s} blocks {len(x):4d} start {us(st.min()):7.2f}..{us(st.max()):7.2f}  "
                  f"kv-landed med +{np.median(kv - st) / 100:5.2f} max {us(kv.max()):7.2f}")
            print(f"{'':12s} scores +{np.median(x[:, 6] - kv) / 100:5.2f} softmax +{np.median(x[:, 7] - x[:, 6]) / 100:5.2f} "
                  f"pv +{np.median(rdy - x[:, 7]) / 100:5.2f}")
            print(f"{'':12s} partial-ready med +{np.median(rdy - kv) / 100:5.2f} max {us(rdy.max()):7.2f}  "
                  f"counted med +{np.median(cnt - rdy) / 100:5.2f} max {us(cnt.max()):7.2f}")
            print(f"{'':12s} combiners {len(lastb)}: burst landed +{np.median(lastb[:, 5] - lastb[:, 3]) / 100:5.2f}  "
                  f"end +{np.median(lastb[:, 4] - lastb[:, 5]) / 100:5.2f}  end max {us(lastb[:, 4].max()):7.2f}")
            e = lastb[:, 4].max()
        else:
            en = x[:, 1]
            print(f"{NAMES[k]:12s} blocks {len(x):4d} start {us(st.min()):7.2f}..{us(st.max()):7.2f}  "
                  f"end {us(en.min()):7.2f}..{us(en.max()):7.2f}  block-dur med {np.median(en - st) / 100:5.2f}")
            e = en.max()
        if k == 0 and len(x) == 512 and (raw0[:512, 1] > 0).all():   # the fused launch's QKV role: q, k and v row blocks
            b = np.arange(512)
            kind = np.where((b & 63) < 32, 0, np.where((b & 63) < 48, 1, 2)) if interleaved else np.where(b < 256, 0, np.where(b < 384, 1, 2))
            print(f"{'':12s} " + "  ".join(f"{nm} blocks end {us(raw0[:512, 1][kind == i].min()):5.2f}..{us(raw0[:512, 1][kind == i].max()):5.2f}"
                                           for i, nm in enumerate("qkv")))
        if k == 1 and len(ch) and wide:
            # the splits' "inputs ready" (mark 1: q -- in the last split k and v too -- normed and the K rows landed)
            # and publish (mark 3) marks: the last split (the new key's), the others, and those of the first chunk
            n = int(ck[ck[:, 1] > ck[:, 0], 2][0])
            nsp = len(x) // 8
            spl = 64 if nsp * 64 >= n else 128
            rows = raw1[:nsp * 8]
            sp = np.arange(nsp * 8) % nsp
            for nm, sel in (("last split", sp == (n - 1) // spl), ("other splits", sp != (n - 1) // spl),
                            ("first chunk", (sp * spl < 256) & (sp != (n - 1) // spl))):
                r = rows[sel & (rows[:, 0] > 0)]
                if len(r):
                    print(f"{'':12s} {nm:12s} ({len(r):3d}): inputs ready {us(np.median(r[:, 1])):5.2f}/{us(r[:, 1].max()):5.2f}  "
                          f"published {us(np.median(r[:, 3])):5.2f}/{us(r[:, 3].max()):5.2f}  (median/max)")
        if prev_end is not None:
            print(f"{'':12s} gap from previous kernel's last block end to first start: {(st.min() - prev_end) / 100:5.2f} us")
        prev_end = e


if __name__ == "__main__":
    main([a for a in sys.argv[1:] if not a.startswith("--")][0], interleaved="--interleaved" in sys.argv)
