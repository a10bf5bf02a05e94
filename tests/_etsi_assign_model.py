"""CPU model of tetra_etsi_assign (TEST INFRASTRUCTURE): the carrier numbering, the event list of a call
(Part A) and the follower with carried state (Part B).

It restates include/tetra_hip.h's description in plain Python on lists and dicts: the events of all groups
are gathered first, each target group then sorts its own (Python's sorted on tuples) and merges them with
its bursts -- no compact list, no rank sort, no selection scan, so it shares no shape with the kernels.
The inputs are the library's arrays (tests/_etsi_sdu_model.build_rows, the sdu / done arrays of
tests/_etsi_sdu_model.expected_arrays, slots and tq as the MAC and traffic calls leave them).
"""
import numpy as np

import _etsi_mac_model as M
import _etsi_sdu_model as S

MAXB, MAXJ, MAXPDU = M.MAXB, M.MAXJ, M.MAXPDU
AE_FIELDS, TA_FIELDS = 16, 8
HOLD_DEFAULT, IDLE_DEFAULT = 720, 72
(E_ROW, E_BURST, E_BLOCK, E_PDU, E_KIND, E_HEAD, E_CARRIER, E_EXT, E_TARGET, E_P_LO, E_P_HI, E_TN, E_FN, E_SSI,
 E_ADDR_TYPE, E_AUX) = range(16)
T_STATE, T_SSI, T_ADDR_TYPE, T_AUX, T_SRC_KEY, T_NALLOC, T_IDLE, T_AGE = range(8)
TCH_NONE, TCH_CONTROL, TCH_FULL, TCH_HALF, TCH_LOST = range(5)
KEY_OFFSET = {0: 0, 1: 1, 2: 2, 3: -1}     # a key's two low bits -> its offset in 6.25 kHz units
EXT_OFFSET = {0: 0, 1: 1, 2: -1, 3: 2}     # the extended bits' offset field -> the same
INACTIVE = [0, -1, 0, -1, -1, 0, 0, 0]     # the ta record of a burst whose timeslot has no entry
NOT_FOLLOWED = [-1, 0, 0, 0, 0, 0, 0, 0]   # ... of a burst that takes no part
SLOT_DTYPE = np.dtype([("since", "<i8"), ("last", "<i8"), ("active", "<i4"), ("ssi", "<i4"), ("addr_type", "<i4"),
                       ("aux", "<i4"), ("src_key", "<i4"), ("head", "<i4"), ("nalloc", "<i4"), ("idle", "<i4")])
STATE_DTYPE = np.dtype([("bit0", "<i8"), ("expired", "<i4"), ("released", "<i4"), ("slot", SLOT_DTYPE, (4,))])


def slots_of(d):
    return (d + 255) // 510   # Python's floor division


def low32(v):
    """The low 32 bits of an integer as an int32."""
    return ((int(v) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def target_key(carrier, ext, own_key):
    """The key an allocation names: ext the 10 extended bits or -1, own_key the sender's key."""
    if ext >= 0:
        return (ext >> 6) * 16000 + 4 * carrier + EXT_OFFSET[(ext >> 4) & 3]
    if own_key < 0:
        return -1
    off = KEY_OFFSET[own_key & 3]
    band = (own_key - off) // 16000
    return band * 16000 + 4 * carrier + off


class Entry:
    def __init__(self):
        self.active = self.since = self.last = self.ssi = self.addr_type = self.aux = 0
        self.src_key = self.head = self.nalloc = self.idle = 0


class State:
    """One carrier's carried state (struct tetra_etsi_assign_state)."""

    def __init__(self, bit0=0):
        self.bit0, self.expired, self.released = int(bit0), 0, 0
        self.slot = [Entry() for _ in range(4)]

    def to_array(self):
        a = np.zeros((), STATE_DTYPE)
        a["bit0"], a["expired"], a["released"] = self.bit0, self.expired, self.released
        for i, e in enumerate(self.slot):
            for name in SLOT_DTYPE.names:
                a["slot"][i][name] = getattr(e, name)
        return a

    def event(self, T, rec, src_key):
        bitmap = (rec[E_HEAD] >> 4) & 15
        for n in (1, 2, 3, 4):
            if not (bitmap >> (4 - n)) & 1:   # the most significant of the four is timeslot 1
                continue
            e = self.slot[n - 1]
            if not e.active:
                e.active, e.since, e.nalloc, e.idle = 1, T, 0, 0
            e.last = T
            e.nalloc += 1
            e.ssi, e.addr_type, e.aux, e.head, e.src_key = rec[E_SSI], rec[E_ADDR_TYPE], rec[E_AUX], rec[E_HEAD], src_key

    def burst(self, p, tn, cls, fn, hold_slots, idle_max):
        """Steps 1 to 3 for a burst that takes part (cls None: no tq); returns its ta record."""
        e = self.slot[tn - 1]
        if e.active and slots_of(p - e.last) > hold_slots:
            e.active = 0
            self.expired += 1
        if not e.active:
            return list(INACTIVE)
        rec = [1, e.ssi, e.addr_type, e.aux, e.src_key, e.nalloc, e.idle, low32(slots_of(p - e.since))]
        if cls in (TCH_FULL, TCH_HALF):
            e.idle, e.last = 0, p
        elif cls == TCH_CONTROL and fn != 18:
            e.idle += 1
            if e.idle > idle_max:
                e.active = 0
                self.released += 1
        return rec


def ordered(g, G, row_bits, nburst, bursts):
    """The live bursts of group g as (pos, row in the group, b), in order."""
    out = []
    for i in range(G):
        c = g * G + i
        for b in range(min(max(int(nburst[c]), 0), MAXB)):
            out.append((i * row_bits + int(bursts[c, b, 0]), i, b))
    return sorted(out)


def events_of(g, bit0, G, row_bits, nburst, bursts, nblock, blocks, npdu, pdus, keep, slots, sdu, maxd, ndone, done, own_key):
    """Part A for one group: [(T, record)] in walk order, every event (recorded or not)."""
    out = []
    nd = min(max(int(ndone[g]), 0), maxd) if maxd > 0 else 0
    for pos, i, b in ordered(g, G, row_bits, nburst, bursts):
        c = g * G + i
        if keep is not None and keep[c, b] == 0:
            continue
        p = bit0 + pos
        for j in range(min(max(int(nblock[c]), 0), MAXJ)):
            kind, crc, bb = (int(v) for v in blocks[c, j, :3])
            if bb != b or crc == 0 or kind not in M.N1:
                continue
            for q in range(min(max(int(npdu[c, j]), 0), MAXPDU)):
                s, pr = [int(v) for v in sdu[c, j, q]], [int(v) for v in pdus[c, j, q]]
                if not s[S.ELEMS] & 4 or s[S.STATUS] != S.OK or pr[0] not in (M.RESOURCE, M.END):
                    continue
                carrier = (s[S.CHAN] >> 16) & 0xFFF
                ext = (s[S.POWER_GRANT] >> 16) & 0x3FF if s[S.ELEMS] & 8 else -1
                if pr[0] == M.RESOURCE:
                    who = [pr[8], pr[7], pr[9]]   # SSI, ADDR_TYPE, AUX of the PDU record
                else:
                    who = [-1, -1, -1]
                    for k in range(nd):
                        d = [int(v) for v in done[g, k]]
                        if d[:4] == [c, b, j, q]:
                            who = [d[S.D_SSI], d[S.D_ADDR_TYPE], d[S.D_AUX]]
                            break
                tn, fn = (int(slots[c, b, 0]), int(slots[c, b, 1])) if slots is not None else (0, 0)
                out.append((p, [c, b, j, q, pr[0], s[S.CHAN] & 0x3FF, carrier, ext, target_key(carrier, ext, own_key),
                                low32(p), p >> 32, tn, fn] + who))
    return out


def run(states, G, row_bits, advance, hold_slots, idle_max, shared_clock, nsym, nburst, bursts, nblock, blocks, npdu, pdus,
        keep, slots, tq, sdu, maxd, ndone, done, row_key, maxe):
    """One tetra_etsi_assign call: states [C / G] State, updated in place.  Returns (nev [C / G], {(g, k): event
    record} for the recorded events, {(c, b): ta record} for every live burst)."""
    C = len(nburst)
    NG = C // G
    streaming = G == 1 and row_bits == 0 and keep is None
    keys = [-1 if row_key is None else int(row_key[g]) for g in range(NG)]
    nev, ev, applying = np.zeros(NG, np.int32), {}, []
    for g in range(NG):
        found = events_of(g, states[g].bit0, G, row_bits, nburst, bursts, nblock, blocks, npdu, pdus, keep, slots, sdu,
                          maxd, ndone, done, keys[g])
        nev[g] = len(found)
        for k, (T, rec) in enumerate(found[:maxe]):
            ev[(g, k)] = rec
            updown, bitmap = (rec[E_HEAD] >> 2) & 3, (rec[E_HEAD] >> 4) & 15
            if rec[E_TARGET] >= 0 and updown in (1, 3) and bitmap != 0:
                applying.append((T, g, k, rec))
    ta = {}
    for t in range(NG):
        st = states[t]
        mine = sorted((T, g, k) for T, g, k, rec in applying
                      if keys[t] >= 0 and rec[E_TARGET] == keys[t] and (g == t or shared_clock))
        at = 0
        for pos, i, b in ordered(t, G, row_bits, nburst, bursts):
            c, p = t * G + i, st.bit0 + pos
            while at < len(mine) and mine[at][0] < p:   # an event at T comes behind every burst with p <= T
                T, g, k = mine[at]
                st.event(T, ev[(g, k)], keys[g])
                at += 1
            tn = int(slots[c, b, 0]) if slots is not None else 0
            cls = None if tq is None else int(tq[c, b, 0])
            if (keep is not None and keep[c, b] == 0) or not 1 <= tn <= 4 or (cls is not None and cls < 0):
                ta[(c, b)] = list(NOT_FOLLOWED)
                continue
            ta[(c, b)] = st.burst(p, tn, cls, int(slots[c, b, 1]), hold_slots, idle_max)
        for T, g, k in mine[at:]:
            st.event(T, ev[(g, k)], keys[g])
        st.bit0 += 2 * max(int(nsym[t]) - 1, 0) if streaming else advance
    return nev, ev, ta


def expected_arrays(nev, ev, ta, ev_out, ta_out):
    """Write what the library writes into copies of the caller's (poisoned) ev and ta arrays."""
    ev_out, ta_out = None if ev_out is None else ev_out.copy(), ta_out.copy()
    for (g, k), rec in ev.items():
        ev_out[g, k] = rec
    for (c, b), rec in ta.items():
        ta_out[c, b] = rec
    return ev_out, ta_out


def state_array(states):
    a = np.zeros(len(states), STATE_DTYPE)
    for i, s in enumerate(states):
        a[i] = s.to_array()
    return a
