"""The group's own host side of the sharded mesh recompute (cvids_amd/csrc/host_group.h: update_meshes_blocking, update_meshes_wait_free,
settle) on hand-built voxel fields, every shard against the oracle on its own view.

tests/test_gpu_group.py runs a group on smooth integrated scenes against the whole-map oracle; tests/test_gpu_shard_fields.py holds the
multi-process twin (cvids_amd/sharded.py) to the per-rank oracle.  Here the fields of tests/voxel_fields.py go into a group
(Chisel(..., shard_block, devices)), a dirty set chosen by the test is made by a sparse depth frame (tests/group_fields.py;
tests/test_group_fields.py shows on the oracle alone what every frame changes and what the cases reach), and after every
UpdateMeshes(force) every array of every job's mesh must equal the owner rank's oracle bit for bit, every other mesh must be untouched,
and chunk count, chunk set and voxels must equal the whole-map oracle's: no ghost stayed, nothing was changed by the recompute.  Which
form a recompute took and which way settle() went is read from the library's own timing lines, in child processes (the hooks are read
once per process)."""
import pytest

from tests import group_fields as gf

pytestmark = pytest.mark.gpu

HOOKS = {"none": {}, "tiny_slots": {"CHISEL_HIP_GROUP_TINY_SLOTS": "1"}, "blocking_mesh": {"CHISEL_HIP_GROUP_BLOCKING_MESH": "1"},
         "threads_0": {"CHISEL_HIP_GROUP_THREADS": "0"}, "mesh_tiny": {"CHISEL_HIP_MESH_TINY": "1"}}


@pytest.fixture
def group(oracle_mod):
    made = []

    def make(case, world, block):
        made.append(gf.GroupField(oracle_mod, gf.CASES[case][0], world, block))
        return made[-1]

    yield make
    for m in made:
        m.close()


def _run(m, case):
    """the turns of a case, then the frame beside the field and an AddChunk per shard -> [(job meshes, vertices) per turn]"""
    out = []
    for name in gf.CASES[case][1]:
        n, nv = m.turn(name)
        assert n > 0 and nv > 0, (case, name)
        out.append((n, nv))
    m.finish()
    return out


# ---- a. every sharding, one turn -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,block", gf.CASES["dense_origin"][2])
@pytest.mark.parametrize("case", ["dense_origin", "dense_far_ids", "thresholds_origin", "thresholds_far_ids"])
def test_every_sharding(group, case, world, block):
    """8^3 chunks, 4^3 of them, at res 0.03, `all`: a world that is no power of two, shard block 1, negative and large chunk ids in the
    owner routing of AddChunk, of the frame and of the segments; 31 of the 93 changed chunks are new and lie outside the block, so most
    job ids and many ghosts are not resident.  The first recompute of a group is the blocking form."""
    assert (world, block) in gf.CASES[case][2]
    (n, nv), = _run(group(case, world, block), case)
    assert n >= 64 and nv > 50000  # (every chunk of the field is a job and has a surface)


# ---- b. turn after turn on one group -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,block", gf.CASES["turns"][2])
def test_turn_after_turn(group, world, block):
    """`corner`, `all`, `line`, `one_inside`, `diagonal` across the origin: turn 1 is blocking, the others wait-free; turn 2 needs far
    more than turn 1's sizes allow and is called off on the device and made again by settle(); the later turns fit, in slots and among
    ghosts of larger turns.  With 8 shards and shard block 2 the small sets leave shards without a job."""
    sizes = _run(group("turns", world, block), "turns")
    assert sizes[1][0] > sizes[0][0] and sizes[1][0] > sizes[2][0]


def _once(runs, key, args, hooks, timeout):
    """a child process started at most once per key: a child that failed, faulted or ran out of time is not started again -- the tests
    that need it fail from what was kept"""
    if key not in runs:
        try:
            runs[key] = gf.run_child(args, hooks, timeout)
        except Exception as e:  # (subprocess.TimeoutExpired: the child hung)
            runs[key] = e
    if isinstance(runs[key], Exception):
        pytest.fail("the child of %s did not end: %r" % (key, runs[key]))
    out, events = runs[key]
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-6000:]
    return out, events


# ---- c. the routes, observed ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route_runs():
    """the five turns of (b) on 8 shards, shard block 1, in a process of its own per hook (`overflow`: the turns of
    test_list_overflow_falls_back, no hook), run once -> the events of every turn"""
    runs = {}

    def run(hook):
        args = {"overflow": ["overflow"], "chain": ["chain", "8", "1"]}.get(hook, ["turns", "8", "1"])
        out, events = _once(runs, hook, args, HOOKS.get(hook, {}), 120)
        turns = [ev for mark, ev in gf.sections(events) if mark.startswith("turn ")]
        print("%s: %s" % (hook, turns))
        return turns

    return run


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_routes_of_settle(route_runs, hook):
    """The child compares everything of every turn; the parent reads which form every recompute took and what settle() saw.  On the
    MI355X (turns `corner`, `all`, `line`, `one_inside`, `diagonal`; B = a blocking line, W = a wait-free line, a number = the status
    word of a settle):
        no hook, CHISEL_HIP_GROUP_THREADS=0, CHISEL_HIP_MESH_TINY=1:  B | W 4 W 0 | W 0 | W 0     | W 4 W 0
        CHISEL_HIP_GROUP_TINY_SLOTS=1:                                B | W 4 W 0 | W 0 | W 4 W 0 | W 4 W 0
        CHISEL_HIP_GROUP_BLOCKING_MESH=1:                             B | B       | B   | B       | B
    Natural sizes give a pure status 4 (turns 2 and 5 need larger slots than the turn before them left) and never another status: the
    hints for jobs and items size grids, they call nothing off.  The fall-back to the blocking form is test_list_overflow_falls_back."""
    turns = route_runs(hook)
    assert len(turns) == 5
    assert turns[0] == [gf.BLOCKING]  # nothing to size the slots from
    if hook == "blocking_mesh":
        assert all(t == [gf.BLOCKING] for t in turns)  # no wait-free line, nothing to settle
        return
    for t in turns[1:]:
        assert t[0] == gf.WAIT_FREE and isinstance(t[1], int), t
        if t[1] == 0:
            assert t == [gf.WAIT_FREE, 0], t
        elif t[1] == 4:
            assert t == [gf.WAIT_FREE, 4, gf.WAIT_FREE, 0], t  # the same recompute again in exact slots, settled at once
        else:
            assert t == [gf.WAIT_FREE, t[1], gf.BLOCKING], t
    assert turns[1][1] != 0  # turn 2 outgrows what turn 1 left: called off by natural sizes
    assert [gf.WAIT_FREE, 0] in turns  # a later turn fits
    if hook == "tiny_slots":
        assert turns[3] == [gf.WAIT_FREE, 4, gf.WAIT_FREE, 0]  # (every other wait-free recompute gets 64-byte slots: `one_inside` would have fitted)


def test_recomputes_back_to_back(route_runs):
    """a checked turn of `all`, then `line`, `one_inside`, `diagonal`, `corner` as IntegrateDepthScan, UpdateMeshes(force) four times with
    no read-out between them, on 8 shards with shard block 1: nothing synchronises the shards but the event chains between consecutive
    recomputes (armed / copied / imported) and the settle at the head of the next frame.  Everything is compared once at the end, every
    job with the last recompute that meshed it.  All four are wait-free, none falls back."""
    first, chain = route_runs("chain")
    assert first == [gf.BLOCKING]
    assert chain.count(gf.WAIT_FREE) >= 4 and gf.BLOCKING not in chain and chain[-1] == 0, chain
    for k, e in enumerate(chain):
        assert e in (gf.WAIT_FREE, 0, 4) and (e != 4 or chain[k + 1:k + 3] == [gf.WAIT_FREE, 0]), chain


@pytest.mark.parametrize("world,block", [(2, 2)])
def test_recomputes_back_to_back_in_process(group, world, block):
    """the same among 2 shards with shard block 2, in this process"""
    m = group("chain", world, block)
    turns = gf.CASES["chain"][1]
    m.turn(turns[0])
    n, nv = m.back_to_back(turns[1:])
    assert n > 0 and nv > 0
    m.finish()


def test_list_overflow_falls_back(route_runs):
    """Neither natural sizes nor a hook make settle() fall back to the blocking form in the turns above: a segment that exceeds its slot is
    status 4, and the other two bits need a dirty list of more than 4096 entries or a plan of more than 32768.  A list that long comes
    without a hook from the set to mesh itself: a wide frame beside the field changes 2358 new chunks, all of them are garbage-collected
    again, and their entries stay as the 5384 ids of their 27-neighbourhoods in one shard's list (tests/test_group_fields.py); the
    frame of `line` in the same turn gives the recompute chunks to mesh.  The wait-free recompute is called off with bit 1, settle()
    doubles the lists (MS.cap) and makes it again the blocking way; the turn after it is wait-free again and fits."""
    turns = route_runs("overflow")
    assert len(turns) == 3 and turns[0] == [gf.BLOCKING] and turns[2] == [gf.WAIT_FREE, 0], turns
    assert len(turns[1]) == 3 and turns[1][0] == gf.WAIT_FREE and turns[1][1] & 1 and turns[1][2] == gf.BLOCKING, turns


def test_every_route_was_taken(route_runs):
    """over the settings: status 0; status 4, a wait-free retry and a status-0 settle; a status that falls back to the blocking form"""
    every = [t for hook in sorted(HOOKS) + ["overflow"] for t in route_runs(hook)]
    assert [gf.WAIT_FREE, 0] in every
    assert [gf.WAIT_FREE, 4, gf.WAIT_FREE, 0] in every
    assert any(len(t) == 3 and t[0] == gf.WAIT_FREE and t[1] not in (0, 4) and t[2] == gf.BLOCKING for t in every)


# ---- d. who settles ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def settle_runs():
    """one child per kind of last turn, started once: every first call of gf.SETTLERS on a group of its own"""
    runs = {}

    def run(when):
        return _once(runs, when, ["settles"] + list(gf.SETTLERS), HOOKS["none" if when == "fits" else "tiny_slots"], 150)

    return run


@pytest.mark.parametrize("who", gf.SETTLERS)
@pytest.mark.parametrize("when", ["fits", "called_off"])
def test_who_settles(settle_runs, when, who):
    """after a wait-free UpdateMeshes the first call into the group is `who`: a reader sees the finished recompute, a writer acts on the
    map after it, Reset leaves an empty group that takes a field and a turn again, close returns -- after a recompute that fits (status
    0) and after one that was called off in 64-byte slots and is made again by that very call (status 4)"""
    out, events = settle_runs(when)
    assert ("ok " + who) in out.stdout.split("\n"), out.stdout[-1500:] + out.stderr[-6000:]
    marks = gf.sections(events)
    (first,) = [ev for mark, ev in marks if mark == "last " + who]  # the wait-free UpdateMeshes and the first call
    (rest,) = [ev for mark, ev in marks if mark == "after " + who]  # everything after it, the checks included
    if who in ("Reset", "close"):  # (the maps are void, and so is the recompute in flight)
        assert first[0] == gf.WAIT_FREE, first
    else:  # settled by the first call itself, not by a later one
        assert first == ([gf.WAIT_FREE, 0] if when == "fits" else [gf.WAIT_FREE, 4, gf.WAIT_FREE, 0]), (first, rest)
    assert rest == [], (first, rest)


# ---- e. larger chunks, no colour, far-reading vertices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chunks_16", "chunks_32", "no_colour"])
def test_other_payloads(group, case):
    """16^3 chunks in a 3^3 block among 3 shards, 32^3 in a 2^3 block among 2 (InterpolateColor's look-ups land inside the map: 317 and
    369 far-reading vertices); a map without colour among 8 (8-byte payloads: the segments carry no colour plane)"""
    (world, block), = gf.CASES[case][2]
    _run(group(case, world, block), case)


@pytest.mark.parametrize("case", sorted(gf.FAR_READING))
def test_far_reading_vertices(group, case):
    """thousands of vertices whose normal or colour is read outside what the shells serve, two turns: the group must answer them as the
    oracle on the rank's view does -- default voxels in a ghost outside its boxes, also in a slot that a larger ghost of the turn before
    held; no chunk where the shard holds none -- not as the whole map would"""
    (world, block), = gf.CASES[case][2]
    m = group(case, world, block)
    for t, name in enumerate(gf.CASES[case][1]):
        exp = m.begin(name)
        far = m.far_reading(exp)
        print("%s turn %d %s: %d far-reading vertices" % (case, t + 1, name, far))
        assert far > gf.FAR_READING[case][t]
        n, nv = m.check(exp)
        assert n > 0 and nv > 0


# ---- f. buffers that regrow ------------------------------------------------------------------------------------------------------------------------------
def test_buffers_that_regrow(group, oracle_mod):
    """send / recv start at 1 MiB: a small turn, a turn whose largest (owner -> shard) segment times the shards exceeds that (asserted
    from the boxes of the definition before anything runs), then a smaller turn in the grown buffers"""
    spec, turns, ((world, block),) = gf.CASES["regrow"]
    side = gf.OracleSide(oracle_mod, spec)
    sizes = []
    for name in turns:
        f = side.frame(name)
        sizes.append(gf.largest_segment_voxels(f.field, spec.N, f.jobs, world, block) * 12 * world)
    assert sizes[0] < (1 << 20) < sizes[1] and sizes[2] < sizes[1], sizes
    _run(group("regrow", world, block), "regrow")
