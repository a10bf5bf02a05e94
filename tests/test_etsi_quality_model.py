"""The link-quality model (tests/_etsi_quality_model.py) on rows built on the CPU: what it reads on
bursts whose corrupted bits are known by construction.  The lower-MAC outputs it scores are the C
oracle's (oracle/etsi.py Receiver.lower_mac), so nothing here needs a GPU; tests/test_gpu_etsi_quality.py
holds the kernel to the same model on the same rows."""
import numpy as np

import _etsi_quality_model as Q
import _lmac_rows as R


def _scored():
    d = Q.built_rows()
    want = R.oracle_rows(d["hard"], d["soft"], d["nsym"], d["cells"])
    o = Q.oracle_outputs(want)
    bq, kq = Q.link_quality(d["soft"], d["hard"], 0, 1, d["cells"], o["nburst"], o["bursts"], o["nblock"],
                            o["blocks"], o["type1"])
    return d, want, o, bq, kq


def test_every_planted_block_still_decodes_to_its_payload():
    """The planted flips and zeros stay inside what the decoder corrects: every burst is found where
    it was placed and every block decodes to the transmitted payload with a good CRC."""
    d, want, _, _, _ = _scored()
    for r, (w, planted, jobs) in enumerate(zip(want, d["planted"], d["jobs"])):
        assert [(s, k) for s, k, _ in w] == planted, r
        for (_, _, dec), job in zip(w, jobs):
            assert len(dec) == len(job)
            for (kind, t1, ok), (jk, pay) in zip(dec, job):
                assert kind == jk and ok and np.array_equal(t1, pay), (r, kind)


def test_records_read_what_was_planted():
    """Clean rows read zero errors and K x amp; e sign flips read NERR = e and WERR = e x amp; t
    training and h head / tail flips read TERR = t and HERR = h; zeroed soft bytes are counted where
    they belong to the block, across SCH/F's gap (+52 from type-5 position 216)."""
    d, _, _, bq, kq = _scored()
    assert len(d["expect"]) > 150
    for r, what, i, f, v in d["expect"]:
        got = int((bq if what == "b" else kq)[r, i, f])
        assert got == v, (r, what, i, f, got, v)


def test_nothing_past_the_counts_and_special_records():
    d, _, o, bq, kq = _scored()
    for c in range(len(d["nsym"])):
        assert (bq[c, o["nburst"][c]:] == Q.POISON).all() and (kq[c, o["nblock"][c]:] == Q.POISON).all()
        assert (bq[c, :o["nburst"][c]] >= 0).all() and (kq[c, :o["nblock"][c]] >= 0).all()
    # a CRC-bad block; a burst outside the row, of kind 7, and a block that names a dead burst
    o = {k: v.copy() for k, v in o.items()}
    stride = d["hard"].shape[1]
    o["blocks"][0, 0, 1] = 0
    o["bursts"][1, 0, 0] = 2 * stride - 509
    o["bursts"][2, 1, 1] = 7
    o["bursts"][3, 0, 0] = -1
    o["blocks"][4, 0, 2] = int(o["nburst"][4])
    bq2, kq2 = Q.link_quality(d["soft"], d["hard"], 0, 1, d["cells"], o["nburst"], o["bursts"], o["nblock"],
                              o["blocks"], o["type1"])
    assert kq2[0, 0].tolist() == [-1, 0, 0, 0]
    for c, b in ((1, 0), (2, 1), (3, 0)):
        assert bq2[c, b].tolist() == [-1] * 4
        js = [j for j in range(o["nblock"][c]) if o["blocks"][c, j, 2] == b]
        assert js and all(kq2[c, j].tolist() == [-1] * 4 for j in js)
    assert kq2[4, 0].tolist() == [-1] * 4
    same = np.ones(kq.shape[:2], bool)
    same[0, 0] = same[4, 0] = False
    for c, b in ((1, 0), (2, 1), (3, 0)):
        same[c, [j for j in range(o["nblock"][c]) if o["blocks"][c, j, 2] == b]] = False
    assert np.array_equal(kq2[same], kq[same])
    # with origin_bits the same rows shifted right read the same
    pad = 6
    soft = np.concatenate([np.full((len(d["nsym"]), 2 * pad), 55, np.int8), d["soft"]], axis=1)
    hard = np.concatenate([np.full((len(d["nsym"]), pad), 1, np.uint8), d["hard"]], axis=1)
    _, _, o0, _, _ = _scored()
    bq3, kq3 = Q.link_quality(soft, hard, 2 * pad, 1, d["cells"], o0["nburst"], o0["bursts"], o0["nblock"],
                              o0["blocks"], o0["type1"])
    assert np.array_equal(bq3, bq) and np.array_equal(kq3, kq)


def test_wrong_cell_reads_many_errors():
    """The record depends on the cell it is given: scored with another init an SCH block reads about
    half its bits wrong, a BSCH block (init 3 whatever the cell) reads the same."""
    d, _, o, bq, kq = _scored()
    _, kq2 = Q.link_quality(d["soft"], d["hard"], 0, 1, d["cells"] ^ np.uint32(0x5A5A5A00), o["nburst"], o["bursts"],
                            o["nblock"], o["blocks"], o["type1"])
    for c in range(2):
        for j in range(o["nblock"][c]):
            kind = int(o["blocks"][c, j, 0])
            if kind == 2:
                assert kq2[c, j].tolist() == kq[c, j].tolist()
            else:
                assert Q.K_OF[kind] // 4 < kq2[c, j, Q.NERR] < 3 * Q.K_OF[kind] // 4
