"""The chunk hash under collisions, tombstones and wrap-around: a restatement of the hash and the key packing, a model of the
open-addressed table, the invariants of a read-out (Chisel.hash_table()), reach predicates on a read-out, and builders of crowded tables.

TEST INFRASTRUCTURE ONLY (tests/test_hash_cases.py checks it on the CPU, tests/test_gpu_hash.py uses it against the device).

The table (cvids_amd/csrc/chisel_device.h): `capacity` buckets, a power of two; a bucket holds KEY_EMPTY, KEY_TOMB or the packed id of a
resident chunk, and beside it the chunk's slot.  Home bucket = ChunkHasher(id) & (capacity - 1), linear probing with wrap-around.
"""
import numpy as np

MASK64 = (1 << 64) - 1
KEY_EMPTY = MASK64
KEY_TOMB = MASK64 - 1
ID_BIAS = 1 << 20
ID_MIN, ID_MAX = -ID_BIAS + 2, ID_BIAS - 2  # the ids every entry accepts, per axis (include/chisel_hip.h)


# ---- a. the hash and the key packing ------------------------------------------------------------------------------------------------
def chunk_hash(x, y, z):
    """ChunkHasher (ChunkManager.h:40-52): size_t arithmetic on sign-extended ints, the third prime 8349279 as the reference has it"""
    return (((int(x) * 73856093) & MASK64) ^ ((int(y) * 19349663) & MASK64) ^ ((int(z) * 8349279) & MASK64)) & MASK64


def pack_id(x, y, z):
    """21 bits per axis, biased by 2^20; no masking (ids outside [-2^20, 2^20) carry into the next field: why they are refused)"""
    u32 = lambda v: (int(v) + ID_BIAS) & 0xFFFFFFFF
    return (u32(x) | (u32(y) << 21) | (u32(z) << 42)) & MASK64


def unpack_id(key):
    key = int(key)
    return ((key & 0x1FFFFF) - ID_BIAS, ((key >> 21) & 0x1FFFFF) - ID_BIAS, ((key >> 42) & 0x1FFFFF) - ID_BIAS)


def home_of(cid, capacity):
    return chunk_hash(*cid) & (capacity - 1)


# ---- b. a model of the table ----------------------------------------------------------------------------------------------------------
class TableModel:
    """insert: first EMPTY or TOMB from home (an id that is resident is found first); remove: the key becomes TOMB; find: stop at
    EMPTY, at most `capacity` probes"""

    def __init__(self, capacity):
        assert capacity & (capacity - 1) == 0
        self.capacity = capacity
        self.keys = [KEY_EMPTY] * capacity

    def find(self, cid):
        key, h = pack_id(*cid), home_of(cid, self.capacity)
        for i in range(self.capacity):
            idx = (h + i) & (self.capacity - 1)
            if self.keys[idx] == key:
                return idx
            if self.keys[idx] == KEY_EMPTY:
                break
        return -1

    def insert(self, cid):
        idx = self.find(cid)
        if idx >= 0:
            return idx
        h = home_of(cid, self.capacity)
        for i in range(self.capacity):
            idx = (h + i) & (self.capacity - 1)
            if self.keys[idx] in (KEY_EMPTY, KEY_TOMB):
                self.keys[idx] = pack_id(*cid)
                return idx
        return -1  # (the table is full of keys)

    def remove(self, cid):
        idx = self.find(cid)
        if idx >= 0:
            self.keys[idx] = KEY_TOMB
        return idx >= 0

    def ids(self):
        return sorted(unpack_id(k) for k in self.keys if k not in (KEY_EMPTY, KEY_TOMB))

    def readout(self):
        """the model as a read-out (keys only), for the reach predicates below"""
        return {"capacity": self.capacity, "hash_keys": np.array(self.keys, np.uint64)}


# ---- c. invariants of a read-out -------------------------------------------------------------------------------------------------------
def resident_keys(t):
    keys = np.asarray(t["hash_keys"], np.uint64)
    return keys[(keys != np.uint64(KEY_EMPTY)) & (keys != np.uint64(KEY_TOMB))]


def resident_ids(t):
    return sorted(unpack_id(k) for k in resident_keys(t))


def check_invariants(t, what=""):
    """the table's contract on a read-out of Chisel.hash_table(); returns the number of resident keys"""
    cap, committed, top = t["capacity"], t["committed"], t["free_top"]
    keys, vals, slot_key, free = (np.asarray(t[k]) for k in ("hash_keys", "hash_vals", "slot_key", "free_list"))
    assert cap & (cap - 1) == 0 and len(keys) == cap and len(vals) == cap and len(slot_key) == committed, what
    assert 0 <= top <= committed and len(free) == top, "%s free_top %d of %d" % (what, top, committed)
    live = np.flatnonzero((keys != np.uint64(KEY_EMPTY)) & (keys != np.uint64(KEY_TOMB)))
    assert len(np.unique(keys[live])) == len(live), "%s a key occurs twice" % what
    for idx in live:
        cid = unpack_id(keys[idx])
        assert pack_id(*cid) == int(keys[idx]), "%s bucket %d: key %x does not unpack to an id" % (what, idx, int(keys[idx]))
        assert all(ID_MIN <= c <= ID_MAX for c in cid), "%s bucket %d: id %s outside the accepted range" % (what, idx, cid)
        h = home_of(cid, cap)
        n = (int(idx) - h) & (cap - 1)  # buckets between home and the key: none of them EMPTY
        path = keys[(h + np.arange(n)) & (cap - 1)]
        assert not (path == np.uint64(KEY_EMPTY)).any(), "%s id %s is cut off from its home %d by an EMPTY bucket" % (what, cid, h)
        v = int(vals[idx])
        assert 0 <= v < committed, "%s id %s: slot %d of %d" % (what, cid, v, committed)
        assert int(slot_key[v]) == int(keys[idx]), "%s id %s: slot %d holds key %x" % (what, cid, v, int(slot_key[v]))
    used = vals[live].astype(np.int64)
    assert len(np.unique(used)) == len(used), "%s two keys share a slot" % what
    assert len(np.unique(free)) == len(free), "%s a slot is on the free list twice" % what
    assert sorted(used.tolist() + free.astype(np.int64).tolist()) == list(range(committed)), "%s used and free slots do not partition the pool" % what
    assert committed - top == len(live), "%s committed %d - free_top %d != %d keys" % (what, committed, top, len(live))
    unused = np.ones(committed, bool)
    unused[used] = False
    assert (slot_key[unused] == np.uint64(KEY_EMPTY)).all(), "%s a free slot carries a key" % what
    return len(live)


# ---- d. reach predicates on a read-out -----------------------------------------------------------------------------------------------
def bucket_of(t, cid):
    """the bucket that holds the id, by a scan of the read-out (no probing: the predicates must not assume what they measure); -1 = absent"""
    at = np.flatnonzero(np.asarray(t["hash_keys"], np.uint64) == np.uint64(pack_id(*cid)))
    return int(at[0]) if len(at) else -1


def probe_length(t, cid):
    """buckets a look-up of a resident id reads: 1 in its home bucket"""
    idx = bucket_of(t, cid)
    assert idx >= 0, cid
    return ((idx - home_of(cid, t["capacity"])) & (t["capacity"] - 1)) + 1


def crosses_end(t, cid):
    idx = bucket_of(t, cid)
    assert idx >= 0, cid
    return idx < home_of(cid, t["capacity"])


def tombstones_on_path(t, cid):
    cap, h = t["capacity"], home_of(cid, t["capacity"])
    path = np.asarray(t["hash_keys"], np.uint64)[(h + np.arange(probe_length(t, cid))) & (cap - 1)]
    return int((path == np.uint64(KEY_TOMB)).sum())


def reach(t, ids):
    """of the ids (all resident): how many sit off their home bucket, have a probe length >= 8, cross the table's end, pass a tombstone"""
    ids = [tuple(int(v) for v in c) for c in ids]
    return {"off_home": sum(probe_length(t, c) > 1 for c in ids), "long": sum(probe_length(t, c) >= 8 for c in ids),
            "cross": sum(crosses_end(t, c) for c in ids), "tomb": sum(tombstones_on_path(t, c) > 0 for c in ids)}


def n_empty(t):
    return int((np.asarray(t["hash_keys"], np.uint64) == np.uint64(KEY_EMPTY)).sum())


def n_tombstones(t):
    return int((np.asarray(t["hash_keys"], np.uint64) == np.uint64(KEY_TOMB)).sum())


# ---- e. builders -----------------------------------------------------------------------------------------------------------------------
_FAR = {}


def _far_by_home(capacity):
    """100 x 40 x 8 ids with coordinates of magnitude 600 ... 1000 on every axis, both signs on every axis, by home bucket: far from
    every scene of the tests (no frame, ray or cloud reaches them), and the box of created ids opens on every side"""
    if capacity not in _FAR:
        by = {}
        for i in range(100):
            x = (600 + i * 37 % 400) * (1 if i % 2 == 0 else -1)  # (odd strides: the low bits of the hash are those of the coordinates)
            for j in range(40):
                y = (600 + j * 97 % 400) * (1 if (j // 2) % 2 == 0 else -1)
                for k in range(8):
                    z = (600 + k * 53 % 400) * (1 if (i + j + k) % 3 == 0 else -1)
                    by.setdefault(home_of((x, y, z), capacity), []).append((x, y, z))
        _FAR[capacity] = by
    return _FAR[capacity]


def far_ids(home, k, capacity=1024, skip=0, owner=None):
    """k far ids whose home bucket is `home` (the same ones on every call; `skip` leaves the first ones out).  owner: a predicate on
    an id -- only the ids it accepts count (a shard takes the chunks it owns only)"""
    pool = _far_by_home(capacity).get(home, [])
    if owner is not None:
        pool = [c for c in pool if owner(c)]
    assert len(pool) >= skip + k, "only %d far ids homed in bucket %d of %d" % (len(pool), home, capacity)
    return pool[skip:skip + k]


def blocker_voxels(k, V, color=False):
    """recognisable voxels of blocker number k: sdf 0.001 (k + voxel index mod 7), weight 1 -- a look-up that lands in the wrong slot
    shows up in the data"""
    i = np.arange(V)
    sdf = (np.float32(0.001) * (k + i % 7).astype(np.float32)).astype(np.float32)
    rgbw = None
    if color:
        rgbw = np.stack([(k + i) % 251, (k // 7 + i) % 241, i % 239, np.ones(V, np.int64)], 1).astype(np.uint8)
    return sdf, np.ones(V, np.float32), rgbw


def colliding_ids(capacity=1024, n=32):
    """n far ids that share 3 homes, one of them the last bucket (its probes wrap), one the first"""
    homes = (capacity - 1, 0, capacity // 2 + 5)
    per = [n - 2 * (n // 3), n // 3, n // 3]
    return [c for h, k in zip(homes, per) for c in far_ids(h, k, capacity)]


def run_across_end(capacity, scene_ids, owner=None):
    """The run across the end: one resident blocker homed in each of the buckets [3/4 cap, cap) and [0, cap / 32), and one more on the
    home of every second chunk the scene will create (scene_ids in the order the oracle creates them: scene_order below).  -> (blockers,
    the ones to remove after the first frames: every second blocker, in the order given).  owner: as for far_ids -- the blockers of one shard's table"""
    run = list(range(3 * capacity // 4, capacity)) + list(range(capacity // 32))
    taken = {}
    blockers = []
    for h in run:
        blockers.append(far_ids(h, 1, capacity, owner=owner)[0])
        taken[h] = 1
    for cid in [tuple(int(v) for v in c) for c in scene_ids][::2]:
        h = home_of(cid, capacity)
        blockers.append(far_ids(h, 1, capacity, skip=taken.get(h, 0), owner=owner)[0])
        taken[h] = taken.get(h, 0) + 1
    return blockers, blockers[::2]


def scene_order(om, frames, cam):
    """the ids of the chunks the frames create in a (fresh) oracle map, in order of creation: frame by frame, within a frame in the
    order the oracle lists them"""
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    order, seen = [], set()
    for depth, pose in frames:
        om.integrate_depth(depth, pose, intr, cam.near_plane, cam.far_plane)
        for c in map(tuple, om.chunk_ids().tolist()):
            if c not in seen:
                seen.add(c)
                order.append(c)
    return order


def saturation_rounds(capacity, fits):
    """one far id per bucket, in rounds of at most `fits` ids: uploaded and collected round by round they leave a tombstone in every
    bucket of an empty table"""
    ids = [far_ids(h, 1, capacity)[0] for h in range(capacity)]
    return [ids[i:i + fits] for i in range(0, capacity, fits)]


def model_run_across_end(capacity, scene_ids, scene_ids_later=()):
    """both steps of the crowded setup on the model, sequential inserts standing in for the frames -> (read-out after the first frames,
    read-out after the removal and the later chunks, blockers, removed)"""
    blockers, removed = run_across_end(capacity, list(scene_ids) + list(scene_ids_later))
    t = TableModel(capacity)
    for b in blockers:
        t.insert(b)
    for c in scene_ids:
        t.insert(tuple(int(v) for v in c))
    before = t.readout()
    for b in removed:
        assert t.remove(b)
    for c in scene_ids_later:
        t.insert(tuple(int(v) for v in c))
    return before, t.readout(), blockers, removed
