"""tests/_etsi_llc_model.py on the CPU: the FCS arithmetic pinned against zlib and the catalogue check value,
and the record rules at their edges.  tests/test_gpu_etsi_llc.py holds the kernels to this model."""
import zlib

import numpy as np
import pytest

import _etsi_mac_model as M
import _etsi_sdu_model as S
import _etsi_llc_model as L


def bitrev(v, n):
    return int(format(v, "0%db" % n)[::-1], 2)


# ------------------------------------------------------------------------------ the CRC, pinned

def test_check_value_of_123456789():
    assert L.fcs(L.bits_of_bytes(b"123456789")) == 0xFC891918


def test_residue_over_a_message_and_its_own_fcs():
    rng = np.random.default_rng(1)
    for n in (0, 1, 7, 8, 33, 236, 4064):
        bits = rng.integers(0, 2, n).tolist()
        assert L.register(bits + M.bits_of(L.fcs(bits), 32)) == L.RESIDUE == 0xC704DD7B, n


def test_zlib_identity_over_random_byte_strings():
    rng = np.random.default_rng(2)
    for n in list(range(0, 40)) + rng.integers(40, 513, 24).tolist() + [512]:
        data = bytes(rng.integers(0, 256, n).astype(np.uint8))
        want = bitrev(zlib.crc32(bytes(bitrev(x, 8) for x in data)), 32)
        assert L.fcs(L.bits_of_bytes(data)) == want, n


# ------------------------------------------------------------------------------ the record rules

NAMED_SEQUENCE = {0: (True, True), 1: (False, True), 2: (False, False), 3: (True, False)}   # has N(R), has N(S)


@pytest.mark.parametrize("t", range(16))
def test_every_type(t):
    rng = np.random.default_rng(10 + t)
    tl = rng.integers(0, 2, 61).tolist()
    for nr in (0, 1):
        for ns in (0, 1):
            rec, got = L.read_pdu(L.llc_pdu(t, tl, nr=nr, ns=ns))
            if t >= 8:
                assert rec == [L.UNSUPPORTED, t, -1, -1, 0, 0, 0, 0, 0, 0] and got == []
                continue
            has_nr, has_ns = NAMED_SEQUENCE[t & 3]
            hdr = 4 + has_nr + has_ns
            assert rec[:6] == [L.OK, t, nr if has_nr else -1, ns if has_ns else -1, hdr, 61] and got == tl
            assert rec[L.HEAD] == M._get(tl, 0, 8)
            if t & 4:
                assert rec[L.FCS] == L.FCS_GOOD and rec[L.FCS_RX] == rec[L.FCS_CALC] != 0
            else:
                assert rec[L.FCS:] == [L.FCS_NONE, 0, 0]


@pytest.mark.parametrize("t", range(8))
def test_every_length_from_0_to_44_bits(t):
    """The malformed edges: below the type (3/4 bits), below the header (4/5, 5/6), below header + 32."""
    rng = np.random.default_rng(30 + t)
    hdr = L.HEADER_BITS[t & 3]
    need = hdr + (32 if t & 4 else 0)
    for n in range(45):
        bits = M.bits_of(t, 4)[:n] + rng.integers(0, 2, max(n - 4, 0)).tolist()
        rec, tl = L.read_pdu(bits)
        if n < need:
            assert rec == [L.MALFORMED, 0, -1, -1, 0, 0, 0, 0, 0, 0] and tl == [], (t, n)
            continue
        assert rec[L.STATUS] == L.OK and rec[L.TYPE] == t and rec[L.OFFSET] == hdr and rec[L.NBITS] == n - need, (t, n)
        assert tl == bits[hdr:hdr + n - need]
        k = n - need
        assert rec[L.HEAD] == (-1 if k < 3 else M._get(tl[:8], 0, min(k, 8)) << (8 - min(k, 8))), (t, n)
        if t & 4:
            assert rec[L.FCS_RX] == M._get(bits, n - 32, 32) and rec[L.FCS_CALC] == L.fcs(bits[:n - 32])
            assert rec[L.FCS] == (L.FCS_GOOD if rec[L.FCS_RX] == rec[L.FCS_CALC] else L.FCS_BAD)
        # the writer's PDU of this length reads good, whatever the length
        if k >= 0:
            rec2, tl2 = L.read_pdu(L.llc_pdu(t, tl, nr=1, ns=0))
            assert rec2[L.STATUS] == L.OK and tl2 == tl and rec2[L.FCS] == (L.FCS_GOOD if t & 4 else L.FCS_NONE)


def test_a_bare_ack_has_zero_bits():
    rec, tl = L.read_pdu(L.llc_pdu(3, [], nr=1))
    assert rec == [L.OK, 3, 1, -1, 5, 0, -1, L.FCS_NONE, 0, 0] and tl == []
    rec, tl = L.read_pdu(L.llc_pdu(7, [], nr=0))
    assert rec[:8] == [L.OK, 7, 0, -1, 5, 0, -1, L.FCS_GOOD] and tl == []


@pytest.mark.parametrize("t,n", [(4, 40), (5, 3), (6, 0), (7, 1), (5, 197)])
def test_one_flipped_bit_anywhere_reads_bad(t, n):
    rng = np.random.default_rng(50 + t)
    tl = rng.integers(0, 2, n).tolist()
    good = L.llc_pdu(t, tl, nr=1, ns=1)
    assert L.read_pdu(good)[0][L.FCS] == L.FCS_GOOD
    for i in range(len(good)):
        rec, _ = L.read_pdu(L.llc_pdu(t, tl, nr=1, ns=1, flip=i))
        # a flip in the type can turn the PDU into one without an FCS, an unsupported or a malformed one:
        # whatever it is, it does not read good
        assert rec[L.FCS] != L.FCS_GOOD, (t, n, i)
        if i >= 4:
            assert rec[L.STATUS] == L.OK and rec[L.FCS] == L.FCS_BAD, (t, n, i)


def pdu_rec(kind=M.RESOURCE, enc=0):
    r = [0] * M.NF
    r[0], r[5] = kind, enc
    return r


def sdu_rec(status=S.OK, nbits=0, byte=0, role=S.WHOLE):
    r = [0] * S.SDU_FIELDS
    r[S.STATUS], r[S.NBITS], r[S.BYTE], r[S.ROLE] = status, nbits, byte, role
    return r


def test_whole_records_none_encrypted_and_offsets():
    rng = np.random.default_rng(70)
    tl = rng.integers(0, 2, 50).tolist()
    bits = L.llc_pdu(6, tl)
    row = np.frombuffer(bytes(rng.integers(0, 256, 3).astype(np.uint8)) + S.pack(bits) + bytes(40), np.uint8)[:40]
    ok = L.read_whole(pdu_rec(), sdu_rec(nbits=len(bits), byte=3), row)
    assert ok[0][:6] == [L.OK, 6, -1, -1, 4, 50] and ok[0][L.FCS] == L.FCS_GOOD and ok[1] == tl
    none, enc = [L.NONE, 0, -1, -1, 0, 0, 0, 0, 0, 0], [L.ENCRYPTED, -1, -1, -1, 0, 0, 0, 0, 0, 0]
    for kind in (M.FRAG, M.END, 3, 4, 5, 6, 7, 8):
        assert L.read_whole(pdu_rec(kind), sdu_rec(nbits=len(bits), byte=3), row) == (none, [])
    for role in (S.FIRST, S.MIDDLE, S.LAST):   # another role: none, even where it is encrypted
        assert L.read_whole(pdu_rec(), sdu_rec(nbits=len(bits), byte=3, role=role), row) == (none, [])
        assert L.read_whole(pdu_rec(enc=1), sdu_rec(S.ENCRYPTED, len(bits), 3, role), row) == (none, [])
    for status in (S.NONE, S.MALFORMED, S.UNSUPPORTED):
        assert L.read_whole(pdu_rec(), sdu_rec(status, len(bits), 3), row) == (none, [])
    assert L.read_whole(pdu_rec(), sdu_rec(nbits=0, byte=3), row) == (none, [])
    assert L.read_whole(pdu_rec(), sdu_rec(S.ENCRYPTED, len(bits), 3), row) == (enc, [])
    assert L.read_whole(pdu_rec(enc=2), sdu_rec(nbits=len(bits), byte=3), row) == (enc, [])
    bad = [L.MALFORMED, 0, -1, -1, 0, 0, 0, 0, 0, 0]
    assert L.read_whole(pdu_rec(), sdu_rec(nbits=len(bits), byte=-1), row) == (bad, [])
    assert L.read_whole(pdu_rec(), sdu_rec(nbits=len(bits), byte=40 - 10), row) == (bad, [])


def test_done_records():
    rng = np.random.default_rng(71)
    tl = rng.integers(0, 2, 4096 - 37).tolist()
    bits = L.llc_pdu(5, tl, ns=1)
    assert len(bits) == 4096
    data = np.frombuffer(S.pack(bits), np.uint8)
    rec = [0] * S.DONE_FIELDS
    rec[S.D_NBITS] = 4096
    got = L.read_done(rec, data)
    assert got[0][:8] == [L.OK, 5, -1, 1, 5, 4096 - 37, M._get(tl, 0, 8), L.FCS_GOOD] and got[1] == tl
    rec[S.D_ENC] = 1
    assert L.read_done(rec, data) == ([L.ENCRYPTED, -1, -1, -1, 0, 0, 0, 0, 0, 0], [])
    rec[S.D_ENC] = 0
    for n, status in ((0, L.NONE), (-1, L.MALFORMED), (4097, L.MALFORMED), (3, L.MALFORMED), (36, L.MALFORMED)):
        rec[S.D_NBITS] = n
        assert L.read_done(rec, data) == ([status, 0, -1, -1, 0, 0, 0, 0, 0, 0], []), n
    rec[S.D_NBITS] = 37
    assert L.read_done(rec, data)[0][:6] == [L.OK, 5, -1, 1, 5, 0]


def test_signed_holds_the_bit_pattern():
    r = L.blank(L.OK)
    r[L.FCS_RX], r[L.FCS_CALC] = 0xFC891918, 0x12345678
    s = L.signed(r)
    assert s[L.FCS_RX] == 0xFC891918 - (1 << 32) and s[L.FCS_CALC] == 0x12345678
