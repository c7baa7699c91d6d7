"""Tables driven through full and incremental publishes, one per leaf geometry -- TEST
INFRASTRUCTURE ONLY (test_publish_states.py on the CPU, test_gpu_publish_states.py on the device).

A State holds a table and the oracle and applies one write script to both in lockstep; every call
asserts that both return the same code.  The script's phases, each followed by a publish in the
GPU test:

  P0 (full)         load four fifths of the key set
  P1 (incremental)  committed updates (chains of 1-2 versions); in-flight updates, some aborted,
                    some updated again by their owner, some finalized; delete and delete_key_owned;
                    every record in slots 64..127 of one leaf deleted (an empty slot group);
                    committed inserts of held-back keys behind the leaves' sorted slots; in-flight
                    inserts, some committed, some aborted (the leaf's count falls), one whose abort
                    is refused because it is no longer the last slot, the rest left in flight
  P2 (incremental)  an in-flight insert of P1, still its leaf's last slot, aborted (the published
                    count falls); P1's in-flight updates committed; a third version on twice-updated
                    rows; every record of one whole leaf deleted (a scan that reaches it ends
                    there); inserts, among them into the leaves with an aborted insert (the slot
                    index is reused); deletes of records P1 inserted
  P3 (full)         held-back keys into the fullest leaves until leaves split
  P4 (incremental)  updates, deletes and inserts on both halves of a leaf that split

Inserts of P1, P2 and P4 go only into leaves with room to spare, so no leaf splits there.  The
leaves before and at the emptied leaf stay out of every random pick, and the emptied leaf and the
leaf with the empty group take no inserts, so those states last to the end.

Device epochs (test_gpu_device_epochs.py; on the CPU the same epochs go through the host's per-key
calls): draw_epoch() draws the ops of one stage_update_batch_device call from every state the
script has made -- live, hot, in-flight, deleted, aborted, held-back and absent keys -- and
device_epoch() applies them to the device and, op by op, to the oracle.  EPOCH_STEPS puts such
epochs between the publishes of the phases; finish_device_flying() lets the host commit and abort
updates the device left in flight.

expected_reads() draws the inputs of every read entry point and computes what the oracle answers
(no device); compare_reads() holds the device against that, exactly; check_all_reads() is both.
"""
import collections
import functools
import zlib

import numpy as np

import oracle_lib as O
import stage
from stage._lib import check
from table_scan_expect import LAST, M_VISIBLE, raw_expect, snapshot_expects
from test_gpu_probe_window import check_status, check_window
from test_gpu_scan_window import check_scan
from test_wide_keys import tpcc_like

M_CONTROL = 1 << 63
PHASES = ("P0", "P1", "P2", "P3", "P4")
INCREMENTAL = ("P1", "P2", "P4")
SCAN_SIZES = (1, 7, 63, 64, 100)  # 63: the last compact size of wide keys / large leaves, 64: the first direct one
FIRST_SIZES = (7, 63)             # index_scan_first: sizes up to 63
KEY_ORDER = functools.cmp_to_key(O.key_compare)
WAVE, LANE = 0, 1                 # stage_set_probe_form


def int_keys(n, mul, add, seed):
    k = np.random.default_rng(seed).permutation(np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(add))
    return [int(x).to_bytes(8, "little") for x in k]


def tpcc_keys(width, n, seed):
    k = tpcc_like(width, n_w=1)[:n]
    return [k[i].tobytes() for i in np.random.default_rng(seed).permutation(n)]


SMALL_LEAVES = dict(leaf_node_size=4096, split_threshold=3072, merge_threshold=1024)    # varlen_family's
LARGE_LEAVES = dict(leaf_node_size=32768, split_threshold=8192, merge_threshold=16384)  # key8_large_leaves'

Epoch = collections.namedtuple("Epoch", "keys deltas wid cid sst window hot hot2 where head_repeat")
# the GPU test's steps (test_gpu_device_epochs.py): the write phases and, between their publishes,
# device epochs -- per epoch (window, sst_mode, head_repeat, old_hot) of State.draw_epoch
EPOCH_STEPS = ("P0", "P1", "E1", "P2", "E2", "E3", "P3", "P4", "E4", "E5")
FINISH_BEFORE = ("P2", "P3")  # phases before which the host finishes updates the epochs left in flight
EPOCH_SEED = 11               # of the generator the epochs are drawn from, on the CPU and on the device
EPOCHS = {
    "E1": [("whole", None, False, False)],
    "E2": [("last", "mixed", True, True)],
    "E3": [("odd", "mixed", False, False), ("odd", None, True, True)],  # back to back on one stream
    "E4": [("bad", "mixed", False, False)],                             # no op may succeed
    "E5": [("whole", "mixed", False, False)],                           # every chunk of the row a second time
}

GEOMETRIES = {
    # name: (key width, payload, table parameters, key set in load order, leaf capacities, key words)
    "ycsb64": (8, 1000, {}, lambda: int_keys(4000, 3, 1, 1), (64,), 1),
    "ycsb128": (8, 600, {}, lambda: int_keys(5000, 3, 1, 2), (128,), 1),
    "varlen128": (0, 8, SMALL_LEAVES, lambda: [str(i).encode() for i in range(5000)], (128,), 1),
    "key8_large": (8, 8, LARGE_LEAVES, lambda: int_keys(7500, 5, 2, 3), (512, 1024), 1),
    "key16_split": (16, 40, {}, lambda: tpcc_keys(16, 7500, 4), (512, 1024), 2),
    "key16_lane": (16, 320, {}, lambda: tpcc_keys(16, 5000, 5), (64, 128, 256), 2),
    "key32": (32, 60, {}, lambda: tpcc_keys(32, 5000, 6), (256, 512, 1024), 4),
}


class Leaf:
    """one reference-format leaf block (the layout table_scan_expect.parse_blocks reads): the meta
    word, key bytes (None where the word is 0) and visibility of every slot below the record count"""

    def __init__(self, block, key_width):
        self.count = (int(block[32:40].view(np.uint64)[0]) >> 44) & 0xFFFF
        self.meta = block[40:40 + 24 * self.count].reshape(self.count, 24)[:, :8].copy().view(np.uint64).reshape(-1)
        self.keys, self.vis = [], np.zeros(self.count, bool)
        for i, m in enumerate(self.meta.tolist()):
            off, klen = (m >> 32) & 0xFFFF, (m & (0x2FFF << 48)) >> 48
            self.keys.append(block[off:off + klen].tobytes() if m else None)
            self.vis[i] = bool(m & M_VISIBLE) and (key_width == 0 or klen == key_width)

    def visible_keys(self, lo=0, hi=None):
        return [self.keys[i] for i in np.nonzero(self.vis)[0] if lo <= i and (hi is None or i < hi)]

    def sorted_keys(self):
        return sorted(self.visible_keys(), key=KEY_ORDER)


class Expected:
    pass


class State:
    def __init__(self, name):
        self.name = name
        self.width, self.payload, params, make_keys, caps, kw = GEOMETRIES[name]
        self.key_pad = (self.width + 7) // 8 * 8 if self.width > 8 else 8
        self.tab = stage.Table(payload_size=self.payload, key_width=self.width, **params)
        self.orc = O.OracleTree(payload_size=self.payload, key_pad=self.key_pad, **params)
        self.cap, self.kw = self.tab.leaf_capacity, self.tab.key_words
        assert self.cap in caps and self.kw == kw, (name, self.cap, self.kw)
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.everything = make_keys()
        hold = set(self.rng.choice(len(self.everything), len(self.everything) // 5, replace=False).tolist())
        self.held = [k for i, k in enumerate(self.everything) if i in hold]  # later inserts land between keys
        self.live = dict.fromkeys(k for i, k in enumerate(self.everything) if i not in hold)
        self.cid, self.cids = 4, []
        self.busy = set()       # keys with an update in flight
        self.deleted, self.inflight, self.aborted, self.abort_counts = [], [], [], []
        self.phase = None
        self.seen, self.stops = set(), 0  # statuses the device returned; scans that ended at the emptied leaf
        self.dev_flying = []    # keys whose update an epoch left in flight, until a host phase finishes them
        self.sst_probes = []    # (key, read id) pairs around the end stamps of an epoch's retired versions
        self.rc_seen = set()    # return codes of the epochs

    # -------------------------------------------------------------------------------- both sides
    def same(self, what, key, a, b):
        assert a == b, (self.name, self.phase, what, key, a, b)
        return a

    def stamp(self):
        """a new writer / commit id, above all earlier ones and two apart from the next"""
        self.cid += 3
        self.cids.append(self.cid)
        return self.cid

    def bytes_(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def delta(self):
        n = min(8, self.payload) // 2
        return int(self.rng.integers(0, self.payload - n + 1)), self.bytes_(n)

    def insert(self, k, cid):
        p = self.bytes_(self.payload)
        rc = self.same("insert", k, self.tab.insert_key(k, p, cid), self.orc.insert(k, len(k), p, cid))
        if rc == stage.RC_OK:
            self.live[k] = None
        return rc

    def insert_inflight(self, k, wid):
        p = self.bytes_(self.payload)
        return self.same("insert_inflight", k, self.tab.insert_key_inflight(k, p, wid),
                         self.orc.insert_inflight(k, len(k), p, wid))

    def commit_insert(self, k, cid):
        rc = self.same("commit_insert", k, self.tab.commit_insert_key(k, cid), self.orc.commit_insert(k, len(k), cid))
        if rc == stage.RC_OK:
            self.live[k] = None
        return rc

    def abort_insert(self, k):
        return self.same("abort_insert", k, self.tab.abort_insert_key(k), self.orc.abort_insert(k, len(k)))

    def abort_last(self, leaf, k):
        """abort the in-flight insert of k, the leaf's last slot; the counts around it are kept"""
        before = self.counts(leaf)
        self.abort_insert(k)
        self.aborted.append(k)
        self.abort_counts.append((before, self.counts(leaf)))

    def flies(self, k, rc):
        if rc == stage.RC_OK:
            self.busy.add(k)
        return rc

    def lands(self, k, rc):
        if rc == stage.RC_OK:
            self.busy.discard(k)
        return rc

    def update(self, k, wid):
        off, d = self.delta()
        return self.flies(k, self.same("update", k, self.tab.update_key(k, off, d, wid),
                                       self.orc.update(k, len(k), off, d, wid)))

    def update_owned(self, k, wid):
        off, d = self.delta()
        return self.same("update_owned", k, self.tab.update_key_owned(k, off, d, wid),
                         self.orc.update_owned(k, len(k), off, d, wid))

    def commit_update(self, k, cid, sst=None):
        sst = cid if sst is None else sst
        return self.lands(k, self.same("commit_update", k, self.tab.commit_update_key(k, cid, sst),
                                       self.orc.commit_update(k, len(k), cid, sst)))

    def abort_update(self, k):
        return self.lands(k, self.same("abort_update", k, self.tab.abort_update_key(k),
                                       self.orc.abort_update(k, len(k))))

    def finalize_update(self, k, cid):
        """the library's finalize_update takes keys of up to 8 bytes only"""
        return self.lands(k, self.same("finalize_update", k,
                                       self.tab.finalize_update(int.from_bytes(k, "little"), cid, len(k)),
                                       self.orc.finalize_update(k, len(k), cid)))

    def gone(self, k, rc):
        if rc in (stage.RC_OK, stage.RC_INVALID):  # RC_INVALID: under the merge threshold, deleted all the same
            self.live.pop(k, None)
            self.deleted.append(k)
            self.busy.discard(k)
        return rc

    def delete(self, k, cid):
        return self.gone(k, self.same("delete", k, self.tab.delete_key(k, cid), self.orc.delete(k, len(k), cid)))

    def delete_owned(self, k):
        return self.gone(k, self.same("delete_owned", k, self.tab.delete_key_owned(k),
                                      self.orc.delete_owned(k, len(k))))

    # -------------------------------------------------------------------------------- the host's view
    def pack(self, keys):
        """key bytes -> the (keys, lens) arguments of Table.probe / range_scan / traverse"""
        if self.kw > 1:
            return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), self.width), None
        words = np.array([int.from_bytes(k, "little") for k in keys], np.uint64)
        return words, (np.array([len(k) for k in keys], np.uint16) if self.width == 0 else None)

    def leaf_of(self, keys):
        words, lens = self.pack(keys)
        return self.tab.traverse(words, lens).tolist()

    def view(self):
        """the host table's leaves in key order, from its reference-format leaf blocks"""
        return [Leaf(b, self.width) for b in self.tab.export_leaf_images()[0]]

    def counts(self, leaf):
        """the leaf's record count on both sides"""
        return int(self.tab.export_leaves()[0][leaf]), int(self.orc.export_leaves(self.cap)[0][leaf])

    def empty_leaves(self, v):
        return [i for i, l in enumerate(v) if l.count > 0 and not l.vis.any()]

    def hole_leaf(self):
        return self.leaf_of([self.hole_key])[0] if self.hole_key else None

    def plan(self, v):
        """the held-back keys of every leaf that may take inserts, and the inserts each leaf has
        room for: LeafNode's NotEnoughSpace test is 40 + (count + 1) * (24 + record) >= leaf size"""
        keys = [k for k in self.held if k not in self.no_insert]
        self.by_leaf = {}
        for k, leaf in zip(keys, self.leaf_of(keys)):
            self.by_leaf.setdefault(leaf, []).append(k)
        limit = (self.tab.leaf_node_size - 41) // (24 + self.key_pad + self.payload)
        self.free = {leaf: limit - v[leaf].count for leaf in self.by_leaf}
        # most room first; 12 and more: every phase's inserts leave three records of room
        self.roomy = sorted((leaf for leaf in self.free if self.free[leaf] >= 12), key=lambda x: (-self.free[x], x))
        assert len(self.roomy) >= 2, (self.name, self.phase, self.free)

    def take(self, leaf, n):
        """up to n held-back keys of the leaf, while it keeps room for three more records"""
        out = []
        while len(out) < n and self.by_leaf.get(leaf) and self.free[leaf] > 3:
            out.append(self.by_leaf[leaf].pop())
            self.free[leaf] -= 1
        taken = set(out)
        self.held = [k for k in self.held if k not in taken]
        return out

    def pick(self, n, avoid=()):
        """n live keys outside the quiet leaves, without an update in flight"""
        pool = [k for k in self.live if k not in self.quiet and k not in self.busy and k not in avoid]
        return [pool[i] for i in self.rng.choice(len(pool), min(n, len(pool)), replace=False)]

    # -------------------------------------------------------------------------------- the script
    def run(self, phase):
        self.phase = phase
        getattr(self, phase.lower())()

    def p0(self):
        cid = self.stamp()
        for k in list(self.live):
            assert self.insert(k, cid) == stage.RC_OK
        v = self.view()
        nl = len(v)
        assert nl >= 8 and nl == self.tab.stats()["leaves"] == self.orc.stats()["leaves"], (self.name, nl)
        e = nl // 2  # the leaf P2 empties; the leaf before it keeps its records
        assert v[e].vis.any() and len(v[e - 1].visible_keys()) >= 5
        self.empty_key = v[e].visible_keys()[0]
        self.hole_key = None
        if self.cap >= 128:  # a leaf with records in slots 64..127 and beside them
            for a in list(range(e + 1, nl - 1)) + list(range(1, e - 1)):
                n = len(v[a].visible_keys(64, 128))
                if n >= 8 and len(v[a].visible_keys()) - n >= 8:
                    self.hole_key = v[a].visible_keys()[0]
                    break
            assert self.hole_key, (self.name, [l.count for l in v])
        where = dict(zip(self.everything, self.leaf_of(self.everything)))
        self.quiet = {k for k, leaf in where.items() if leaf in (e - 1, e)}
        self.no_insert = self.quiet | {k for k, leaf in where.items() if leaf == self.hole_leaf()}

    def p1(self):
        v = self.view()
        self.plan(v)
        if self.hole_key:
            cid = self.stamp()
            for k in v[self.hole_leaf()].visible_keys(64, 128):
                self.delete(k, cid)
        hot = self.pick(200)
        for ks in (hot, hot[:100]):  # chains of 1-2 versions
            wid, cid = self.stamp(), self.stamp()
            for k in ks:
                self.update(k, wid)
                self.commit_update(k, cid)
        self.twice = hot[:100]
        fly = self.pick(60, avoid=set(hot))
        wid = self.stamp()
        for k in fly:
            self.update(k, wid)
        for k in fly[:15]:
            self.abort_update(k)
        for k in fly[15:30]:
            self.update_owned(k, wid)
        self.flying = fly[15:30] + fly[45:]
        if self.width <= 8:
            cid = self.stamp()
            for k in fly[30:45]:
                self.finalize_update(k, cid)
        else:
            self.flying += fly[30:45]
        self.busy = set(self.flying)
        cid = self.stamp()
        rest = self.pick(90)
        for k in rest[:60]:
            self.delete(k, cid)
        for k in rest[60:]:
            self.delete_owned(k)
        # in-flight inserts.  Three leaves take one that is aborted and nothing else (the publish
        # sees the count back where it was and the slot cleared; P2 uses the slot again), one leaf
        # takes one that stays its last slot (P2 aborts it: the published count falls)
        assert len(self.roomy) >= 5, (self.name, self.free)
        spare, lone, rest = self.roomy[-3:], self.roomy[-4], self.roomy[:-4]
        wid, cid = self.stamp(), self.stamp()
        for leaf in spare:
            k, = self.take(leaf, 1)
            self.insert_inflight(k, wid)
            self.abort_last(leaf, k)
        # ... an abort refused because another insert follows in the leaf ...
        k, k2 = self.take(rest[0], 2)
        self.insert_inflight(k, wid)
        self.insert(k2, cid)
        self.refused_rc = self.abort_insert(k)
        self.inflight.append(k)
        # ... committed, or left in flight (in the leaves with the most room, the last P3 would split)
        ks = [k for i in (1, 2, 3, 0, 1, 2) for k in self.take(rest[i % len(rest)], 1)]
        for k in ks:
            self.insert_inflight(k, wid)
        for k in ks[:3]:
            self.commit_insert(k, cid)
        self.inflight += ks[3:]
        self.inserted_p1 = ks[:3] + [k2]
        for leaf in rest:  # committed inserts: out-of-order slots behind the leaves' sorted ones
            for k in self.take(leaf, 3):
                self.insert(k, cid)
                self.inserted_p1.append(k)
        self.lone_key, = self.take(lone, 1)
        self.insert_inflight(self.lone_key, wid)
        self.inflight.append(self.lone_key)

    def p2(self):
        self.inflight.remove(self.lone_key)
        self.abort_last(self.leaf_of([self.lone_key])[0], self.lone_key)
        v = self.view()
        self.plan(v)
        cid = self.stamp()
        for k in self.flying:
            self.commit_update(k, cid)
        wid, cid = self.stamp(), self.stamp()
        for k in self.twice[:40]:
            self.update(k, wid)
            self.commit_update(k, cid)
        cid = self.stamp()
        for k in v[self.leaf_of([self.empty_key])[0]].visible_keys():
            self.delete(k, cid)
        cid = self.stamp()
        for leaf in sorted(set(self.leaf_of(self.aborted))):  # the slot index an abort freed is used again
            for k in self.take(leaf, 1):
                self.insert(k, cid)
        for leaf in self.roomy:
            for k in self.take(leaf, 2):
                self.insert(k, cid)
        cid = self.stamp()
        for k in self.inserted_p1[::2]:
            self.delete(k, cid)

    def p3(self):
        v = self.view()
        self.plan(v)
        leaves0 = self.tab.stats()["leaves"]
        cid = self.stamp()
        fed = []
        for leaf in sorted(self.free, key=lambda x: (self.free[x], x)):  # least room first
            ks = self.by_leaf.pop(leaf)
            for k in ks:
                self.insert(k, cid)
            taken = set(ks)
            self.held = [k for k in self.held if k not in taken]
            fed.append(v[leaf].visible_keys() + ks)
            if self.tab.stats()["leaves"] > leaves0 and len(fed) >= 2:
                break
        # a split keeps the visible records and clears their control bit: an insert in flight in a
        # leaf that split is committed by it
        flying = {k for l in self.view() for k, m in zip(l.keys, l.meta.tolist()) if m & M_CONTROL}
        for k in [k for k in self.inflight if k not in flying]:
            self.inflight.remove(k)
            self.live[k] = None
        self.busy &= flying  # ... and so is an update in flight there (its copy stays behind the record)
        self.dev_flying = [k for k in self.dev_flying if k in self.busy]
        self.halves = None
        for ks in fed:  # a fed leaf whose keys now route to two leaves has split
            ids = self.leaf_of(ks)
            if len(set(ids)) >= 2:
                self.halves = [[k for k, i in zip(ks, ids) if i == u] for u in sorted(set(ids))[:2]]
                break

    def p4(self):
        v = self.view()
        self.plan(v)
        wid, cid, cid2 = self.stamp(), self.stamp(), self.stamp()
        for half in self.halves:
            ks = [k for k in half if k in self.live and k not in self.busy]
            ks = [ks[i] for i in self.rng.choice(len(ks), min(30, len(ks)), replace=False)]
            for k in ks[:20]:
                self.update(k, wid)
                self.commit_update(k, cid)
            for k in ks[20:28]:
                self.delete(k, cid2)
            for k in ks[28:]:
                self.update(k, wid)
                self.busy.add(k)
        for leaf in self.roomy[:4]:
            for k in self.take(leaf, 1):
                self.insert(k, cid2)

    # -------------------------------------------------------------------------------- device epochs
    def window(self, kind):
        """the (payload offset, length) every op of an epoch patches"""
        p = self.payload
        return {"whole": (0, p), "last": (p - 1, 1), "odd": (5, 151) if p >= 156 else (1, p - 3),
                "bad": (p - 1, 4)}[kind]  # bad: past the payload's end

    def column(self, k, window):
        """the record's current bytes of the window, as the leaf holds them (in flight or not)"""
        _, rec = self.orc.read(k, len(k), for_update=True)
        return rec[self.key_pad + window[0]:self.key_pad + sum(window)].tobytes()

    def neighbours(self, rng, calm):
        """two keys of `calm` in neighbouring slots of one leaf"""
        v = self.view()
        for a in rng.permutation(len(v)).tolist():
            l = v[a]
            for i in range(l.count - 1):
                if l.vis[i] and l.vis[i + 1] and l.keys[i] in calm and l.keys[i + 1] in calm:
                    return [l.keys[i], l.keys[i + 1]]
        raise AssertionError((self.name, "no two calm keys in neighbouring slots"))

    def draw_epoch(self, rng, m, window, sst_mode, head_repeat=False, old_hot=False, avoid=()):
        """One epoch of m ops that all patch `window` -> Epoch(keys, deltas, wid, cid, sst, ...);
        nothing touches the device.  The ops, in random batch order:
          * a hot key 200 times, deltas of a 3-letter alphabet (OK and NOT_NEEDED_UPDATE interleave:
            at least kJumpFrom = 128 ops follow its first failure, the pointer-jump finisher's
            groups; with old_hot some of its writers are older than the record and the group is
            walked instead); head_repeat: its first op repeats the record's current column;
          * a second hot key 70 times (the wave finisher, across a 64-op chunk), op 35 succeeds and
            is left uncommitted: the rest of the group is DIRTY;
          * two keys in neighbouring slots of one leaf 40 times each (two groups in one chunk);
          * every in-flight insert and 40 keys with a host update in flight (DIRTY);
          * deleted, aborted, held-back and absent keys (NOT_FOUND), and for variable-length keys
            ten live keys with a trailing zero byte: the same key word, another length (NOT_FOUND);
          * live keys at random for the rest (about two thirds of m): a tenth left uncommitted, a
            twentieth with the record's current column as their delta (NOT_NEEDED_UPDATE);
          * about 3 % of all ops with writer id 1 (NOT_NEEDED_UPDATE by cstamp).
        Ids: wid = b + 4 i, cid = wid + 2 (0: uncommitted); sst_mode None passes no end stamps,
        "mixed" one of cid - 2, cid - 1, cid, cid + 1 per op (never 0).  cid - 2 is the only one
        of them with a read id strictly between end stamp and commit id (ids are integers): reads
        at cid - 1 miss the chain there, and sst_probes collects those.  Every id goes to
        self.cids.  avoid: keys the hot picks leave out (those of an epoch drawn before this one and
        not yet applied, which may change their column or leave them in flight)."""
        off, ln = window
        bad = off + ln > self.payload
        pool = [k for k in self.live if k not in self.quiet]
        calm = {k for k in pool if k not in self.busy and k not in avoid}
        pair = self.neighbours(rng, calm)
        rest = sorted(calm - set(pair))
        hot, hot2 = (rest[i] for i in rng.choice(len(rest), 2, replace=False))
        letters = [bytes([c]) * ln for c in rng.choice(256, 3, replace=False).tolist()]
        ops = []  # [key, delta, committed, may take writer id 1, (group, index in it) of the hot groups' ops]
        seq = rng.integers(0, 3, 200).tolist()
        ops += [[hot, letters[c], True, old_hot, ("hot", j)] for j, c in enumerate(seq)]
        if head_repeat and not bad:
            ops[0][1] = self.column(hot, window)
        seq = rng.integers(0, 3, 70).tolist()
        seq[35] = (seq[34] + 1) % 3  # differs from the column the ops before it left: succeeds
        ops += [[hot2, letters[c], j != 35, False, ("hot2", j)] for j, c in enumerate(seq)]
        for k in pair:
            ops += [[k, letters[c], True, True, None] for c in rng.integers(0, 3, 40).tolist()]
        others = (self.inflight + self.some(rng, sorted(self.busy), 40) + self.some(rng, self.deleted, 60)
                  + self.aborted + self.some(rng, self.held, 60) + [self.absent_key(rng) for _ in range(60)])
        if self.width == 0:
            others += [k + b"\0" for k in self.some(rng, [k for k in pool if len(k) < 8], 10)]
        ops += [[k, self.bytes_rng(rng, ln), True, True, None] for k in others]
        pool = [k for k in pool if k not in (hot, hot2, *pair)]
        for k in (pool[i] for i in rng.integers(0, len(pool), max(m - len(ops), 0))):
            u = rng.random()
            d = self.column(k, window) if u < 0.05 and not bad else self.bytes_rng(rng, ln)
            ops.append([k, d, not 0.05 <= u < 0.15, True, None])
        ops = [ops[i] for i in self.keep_order(rng, ops)]
        n = len(ops)
        b = (self.cid + 8) // 4 * 4
        self.cid = b + 4 * n + 4
        wid = (b + 4 * np.arange(n)).astype(np.uint32)
        cid = wid + np.uint32(2)
        old = (rng.random(n) < 0.03) & np.array([o[3] for o in ops])
        sst = None
        used = set(wid.tolist()) | set(cid.tolist())
        if sst_mode == "mixed":
            sst = (cid.astype(np.int64) + rng.integers(-2, 2, n)).astype(np.uint32)
            used |= set(sst.tolist())
        else:
            assert sst_mode is None, sst_mode
        self.cids += sorted(used)
        wid[old] = 1
        cid[~np.array([o[2] for o in ops])] = 0
        deltas = np.frombuffer(b"".join(o[1] for o in ops), np.uint8).reshape(n, ln)
        where = {o[4]: i for i, o in enumerate(ops) if o[4]}
        return Epoch([o[0] for o in ops], deltas, wid, cid, sst, window, hot, hot2, where, head_repeat and not bad)

    def bytes_rng(self, rng, n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def keep_order(self, rng, ops):
        """a random batch order that keeps each key's ops in the order drawn"""
        pos = rng.permutation(len(ops)).tolist()  # the batch positions dealt out, one per op
        by_key = collections.defaultdict(list)
        for i, o in enumerate(ops):
            by_key[o[0]].append(i)
        out = [None] * len(ops)
        for drawn in by_key.values():  # the key's positions, lowest first, take its ops as drawn
            for at, i in zip(sorted(pos[j] for j in drawn), drawn):
                out[at] = i
        return out

    def epoch_on_oracle(self, ep):
        """the epoch applied to the oracle op by op -> its return codes"""
        off = ep.window[0]
        rc = np.zeros(len(ep.keys), np.uint8)
        for i, k in enumerate(ep.keys):
            r = self.orc.update(k, len(k), off, ep.deltas[i].tobytes(), int(ep.wid[i]))
            if r == stage.RC_OK and ep.cid[i]:
                r = self.orc.commit_update(k, len(k), int(ep.cid[i]), int(ep.cid[i] if ep.sst is None else ep.sst[i]))
            rc[i] = r
        return rc

    def note_epoch(self, ep, codes):
        """the State's books after an epoch with these codes"""
        self.rc_seen |= set(codes.tolist())
        for i in np.nonzero((codes == stage.RC_OK) & (ep.cid == 0))[0]:
            self.busy.add(ep.keys[i])
            self.dev_flying.append(ep.keys[i])
        if ep.sst is not None:  # retired versions that end two ids before the commit
            gap = np.nonzero((codes == stage.RC_OK) & (ep.cid != 0) & (ep.sst + np.uint32(2) == ep.cid))[0]
            at = gap[np.linspace(0, gap.size - 1, min(gap.size, 40)).astype(int)] if gap.size else gap
            self.sst_probes += [(ep.keys[i], int(ep.cid[i]) - d) for i in at for d in (1, 2)]
        return codes

    def same_codes(self, what, ep, rc, exp):
        bad = np.nonzero(rc != exp)[0]
        assert bad.size == 0, (self.name, what, bad.size, [(int(i), ep.keys[i], int(rc[i]), int(exp[i]),
                                                            int(ep.wid[i]), int(ep.cid[i])) for i in bad[:8]])

    def device_args(self, ep):
        """the epoch's arguments of update_batch_device, after the keys: their lens last"""
        words, lens = self.pack(ep.keys)
        return words, (ep.window[0], ep.deltas, ep.wid, ep.cid, ep.sst, lens)

    def device_epoch(self, ep):
        """the epoch applied by the device and, op by op, by the oracle: equal codes"""
        words, rest = self.device_args(ep)
        rc, n_ok = self.tab.update_batch_device(words, *rest)
        exp = self.epoch_on_oracle(ep)
        self.same_codes("device epoch", ep, rc, exp)
        assert n_ok == int((exp == stage.RC_OK).sum()), (self.name, n_ok)
        return self.note_epoch(ep, exp)

    def device_epochs_pipelined(self, eps):
        """the epochs enqueued back to back on one stream, no host wait between them"""
        s = stage.Stream()
        calls = []
        for ep in eps:
            words, (off, deltas, wid, cid, sst, lens) = self.device_args(ep)
            words = self.tab.key_buffer(words)[0]
            d = [None if a is None else stage.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
                 for a in (words, lens, deltas.reshape(-1), wid, cid, sst)]
            ptr = [None if x is None else x.ptr for x in d]
            rcb = stage.DeviceBuffer(len(ep.keys))
            check(stage.lib().stage_update_batch_device(self.tab.h, ptr[0], ptr[1], len(ep.keys), off, ptr[2],
                                                        deltas.shape[1], ptr[3], ptr[4], ptr[5], rcb.ptr, None, s.ptr),
                  "update_batch_device")
            calls.append((ep, rcb, d))
        s.sync()
        out = []
        for ep, rcb, _ in calls:
            exp = self.epoch_on_oracle(ep)
            self.same_codes("pipelined epoch", ep, rcb.to_numpy(np.uint8, len(ep.keys)), exp)
            out.append(self.note_epoch(ep, exp))
        return out

    def apply_epoch_on_host(self, ep):
        """the same epoch through the host's per-key calls, and the oracle's -> the codes"""
        off = ep.window[0]
        rc = np.zeros(len(ep.keys), np.uint8)
        for i, k in enumerate(ep.keys):
            d, w, c = ep.deltas[i].tobytes(), int(ep.wid[i]), int(ep.cid[i])
            r = self.same("epoch update", k, self.tab.update_key(k, off, d, w), self.orc.update(k, len(k), off, d, w))
            if r == stage.RC_OK and c:
                sst = c if ep.sst is None else int(ep.sst[i])
                r = self.same("epoch commit", k, self.tab.commit_update_key(k, c, sst),
                              self.orc.commit_update(k, len(k), c, sst))
            rc[i] = r
        return self.note_epoch(ep, rc)

    def finish_device_flying(self, rng):
        """the host finishes updates whose copy headers the device wrote: half of those the epochs
        left in flight are committed, a quarter aborted, the rest stay in flight"""
        ks = [k for k in dict.fromkeys(self.dev_flying) if k in self.busy]
        ks = [ks[i] for i in rng.permutation(len(ks))]
        cid = self.stamp()
        for k in ks[:len(ks) // 2]:
            assert self.commit_update(k, cid) == stage.RC_OK, k
        for k in ks[len(ks) // 2:3 * len(ks) // 4]:
            assert self.abort_update(k) == stage.RC_OK, k
        self.dev_flying = []
        return len(ks)

    def draw_step(self, rng, step, m=2000):
        """the epochs of one step of EPOCH_STEPS, drawn before any of them is applied"""
        eps = []
        for kind, sst_mode, head_repeat, old_hot in EPOCHS[step]:
            avoid = {k for ep in eps for k in ep.keys}
            eps.append(self.draw_epoch(rng, m, self.window(kind), sst_mode, head_repeat, old_hot, avoid))
        return eps

    # -------------------------------------------------------------------------------- the oracle's answers
    def read_id_pool(self):
        """read ids below, at and above every commit id used, 0, and the newest"""
        return np.array(sorted({c + d for c in self.cids for d in (-1, 0, 1)} | {0, LAST}), np.uint32)

    def absent_key(self, rng):
        if self.width == 0:
            return str(int(rng.integers(5000, 100000))).encode()
        if self.width == 8:
            return int(rng.integers(0, 1 << 62)).to_bytes(8, "little")
        return rng.integers(0, 256, self.width, dtype=np.uint8).tobytes()

    def some(self, rng, keys, n):
        return [keys[i] for i in rng.choice(len(keys), min(n, len(keys)), replace=False)] if keys else []

    def oracle_reads(self, keys, rids):
        out = np.zeros(len(keys), O.READ_OUT_DTYPE)
        rec = np.zeros((len(keys), self.orc.row), np.uint8)
        for i, k in enumerate(keys):
            out[i], rec[i] = self.orc.read(k, len(k), LAST if rids is None else int(rids[i]))
        return out, rec

    def oracle_scans(self, starts, size, rids=None):
        """orc.scan (rids None) or orc.index_scan per start -> counts, rows (zero past the count)[, status]"""
        n = len(starts)
        counts, rows = np.zeros(n, np.uint32), np.zeros((n, size, self.orc.row), np.uint8)
        status = np.zeros((n, size), np.uint8)
        for i, k in enumerate(starts):
            if rids is None:
                c, r = self.orc.scan(k, len(k), size)
            else:
                c, r, status[i, :c] = self.orc.index_scan(k, len(k), size, int(rids[i]))
            counts[i], rows[i, :c] = c, r
        return (counts, rows) if rids is None else (counts, rows, status)

    def expected_reads(self, rng):
        """the inputs of every read entry point and the oracle's answers; no device is touched"""
        x = Expected()
        x.view = v = self.view()
        pool = self.read_id_pool()
        # probes: present, absent (held back), deleted, in-flight-inserted, aborted and random keys
        x.keys = (self.some(rng, self.everything, 200) + self.some(rng, self.deleted, 40) + self.inflight
                  + self.aborted + self.some(rng, sorted(self.busy), 20) + [self.absent_key(rng) for _ in range(20)])
        x.rids = rng.choice(pool, len(x.keys)).astype(np.uint32)
        x.keys += [k for k, _ in self.sst_probes]  # just below and inside the gap end stamp .. commit id
        x.rids = np.concatenate([x.rids, np.array([r for _, r in self.sst_probes], np.uint32)])
        x.reads = {True: self.oracle_reads(x.keys, x.rids), False: self.oracle_reads(x.keys, None)}
        n = self.payload // 2
        x.window = (n, min(7, self.payload - n))
        # scans: random and deleted keys, the table's first and last key, the last five keys of the
        # leaf before an emptied leaf, the first key of the leaf with the empty slot group
        x.starts = self.some(rng, self.everything, 100) + self.some(rng, self.deleted, 15)
        x.starts += [v[0].sorted_keys()[0], max((k for l in v[-2:] for k in l.visible_keys()), key=KEY_ORDER)]
        x.empty = self.empty_leaves(v)
        x.five = []
        for e in x.empty:
            assert any(l.vis.any() for l in v[e + 1:])  # larger keys exist
            x.five.append(list(range(len(x.starts), len(x.starts) + 5)))
            x.starts += v[e - 1].sorted_keys()[-5:]
        if self.hole_key:
            x.starts.append(v[self.hole_leaf()].sorted_keys()[0])
        x.srids = rng.choice(pool, len(x.starts)).astype(np.uint32)
        x.scans = {size: self.oracle_scans(x.starts, size) for size in SCAN_SIZES}
        x.iscans = {size: self.oracle_scans(x.starts, size, x.srids) for size in SCAN_SIZES}
        # index_scan_first with one prefix word: the index scan up to its first LATEST / OLD
        # record that carries the start key's first eight bytes
        x.first = {}
        for size in FIRST_SIZES if self.width else ():
            ic, irows, ist = x.iscans[size]
            exp = np.zeros(len(x.starts), np.uint8)
            for i, k in enumerate(x.starts):
                for j in range(ic[i]):
                    if ist[i, j] in (stage.ST_LATEST, stage.ST_OLD) and irows[i, j, :8].tobytes() == k[:8]:
                        exp[i] = ist[i, j]
                        break
            x.first[size] = exp
        # whole-table scans: raw and at two read ids, the whole table and around the emptied leaf
        x.raw = raw_expect(self.orc, kwords=self.kw)
        x.trids = (LAST, self.cids[len(self.cids) // 2])
        x.snap = snapshot_expects(self.orc, x.raw, self.width, x.trids)
        nl = x.raw.leaves
        assert nl == len(v)
        e = x.empty[0] if x.empty else nl // 2
        x.ranges = [(0, nl), (e - 1, e + 2)]
        return x

    # -------------------------------------------------------------------------------- the device
    def compare_reads(self, x):
        tab, orc, row = self.tab, self.orc, self.orc.row
        words, lens = self.pack(x.keys)
        o_meta = orc.export_leaves(self.cap)[2]
        for with_rids in (True, False):
            rids = x.rids if with_rids else None
            o_out, o_rec = x.reads[with_rids]
            out, rows = tab.probe(words, read_ids=rids, lens=lens)
            check_status(out, o_out)
            assert np.array_equal(rows[:, :row], o_rec) and not rows[:, row:].any()
            hit = np.nonzero(out["status"] != stage.ST_NOT_FOUND)[0]  # the hit slot's RecordMetadata word
            meta = (out["meta_hi"][hit].astype(np.uint64) << np.uint64(32)) | out["rec_cstamp"][hit].astype(np.uint64)
            assert np.array_equal(meta, o_meta[out["leaf"][hit], out["slot"][hit]])
            self.seen |= set(np.unique(out["status"]).tolist())
            out_w, win = tab.probe(words, read_ids=rids, lens=lens, window=x.window)
            assert out_w.tobytes() == out.tobytes()
            check_window(win, o_rec, self.key_pad, x.window)
            assert np.array_equal(win[:, :x.window[1]],
                                  rows[:, self.key_pad + x.window[0]:self.key_pad + sum(x.window)])
            if self.name in ("ycsb64", "ycsb128"):  # the wave-per-probe form writes the same bytes
                try:
                    tab.set_probe_form(WAVE)
                    out0, rows0 = tab.probe(words, read_ids=rids, lens=lens)
                    bare0, _ = tab.probe(words, read_ids=rids, lens=lens, records=False)
                finally:
                    tab.set_probe_form(LANE)  # the default
                assert out0.tobytes() == out.tobytes() == bare0.tobytes() and np.array_equal(rows0, rows)
        for le in (True, False):
            assert np.array_equal(tab.resolve(words, lens, le_child=le), tab.traverse(words, lens, le_child=le))

        words, lens = self.pack(x.starts)
        for size in SCAN_SIZES:
            oc, orows = x.scans[size]
            counts, rows = tab.range_scan(words, size, lens=lens)
            assert np.array_equal(counts, oc), (size, np.nonzero(counts != oc)[0][:5], counts[counts != oc][:5])
            assert np.array_equal(rows[:, :, :row], orows), size
            check_scan(tab.range_scan(words, size, lens=lens, window=x.window, row_keys=True), oc, orows,
                       self.key_pad, x.window, rows)
            for five in x.five:  # fewer records than asked for although larger keys exist
                self.stops += int((counts[five] < size).sum())
            ic, irows, ist = x.iscans[size]
            counts, rows, status = tab.index_scan(words, size, read_ids=x.srids, lens=lens)
            assert np.array_equal(counts, ic), (size, np.nonzero(counts != ic)[0][:5])
            assert np.array_equal(status, ist), size
            assert np.array_equal(rows[:, :, :row], irows), size
            self.seen |= set(np.unique(status[np.arange(size)[None, :] < counts[:, None]]).tolist())
        for size, exp in x.first.items():
            image, status = tab.index_scan_first(words, size, 1, read_ids=x.srids)
            assert np.array_equal(status, exp), (size, np.nonzero(status != exp)[0][:5])
            assert np.array_equal(image == 0xFFFFFFFF, status == 0)

        for rid in (None,) + x.trids:
            e = x.raw if rid is None else x.snap[rid]
            for a, b in x.ranges:
                total, offsets, meta, status, rows = e.range(a, b)
                got = tab.table_scan(leaves=(a, b), read_id=rid, row_meta=True)
                what = (rid, a, b)
                assert got.count == total, what
                assert np.array_equal(got.offsets, offsets), what
                assert np.array_equal(got.meta, meta), what
                assert np.array_equal(got.status, status), what
                assert np.array_equal(got.records[:, :row], rows), what



def check_all_reads(state, rng):
    """every read entry point of the published table against the oracle"""
    state.compare_reads(state.expected_reads(rng))
