"""The host arithmetic of the emulator trainer (nautilus_amd/csrc/
nb_train_plan.h, the very header nb_mlp_train.hip includes), built for the
host by tests/train_plan_check.cpp: which workgroup updates which weight tile
in the gradient phase, where a weight lives in the tile-major buffers, which
XCDs a resident trainer owns, the layout of its device memory and the steps
of an epoch.

``g_job`` of the trainer has a body for five block shapes and runs a record
of any other shape as 1 x 1, leaving tiles without their Adam step: the
planner must emit only those shapes and cover every tile exactly once."""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'train_plan.json')

H = (100, 50, 20, 1)                     # outputs of the four layers
HT = (7, 4, 2, 1)                        # ... in 16-wide tiles
SHAPES = {(1, 1), (2, 1), (1, 2), (3, 1), (2, 2)}    # (nk, nh) g_job runs


def layer_tiles(kt1):
    """(k-tiles, h-tiles) of the four layers"""
    return list(zip((kt1,) + HT[:3], HT))


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    path = str(tmp_path_factory.mktemp('train_plan') / 'train_plan_check')
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2',
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'train_plan_check.cpp'), '-o', path])
    return path


@pytest.fixture(scope='module')
def consts(exe):
    """the header's constants by name: XCD_SLOTS, G_ROWT, the bytes of the
    slots nb_trainer_create_fleet checks the job lists against, ..."""
    out = subprocess.check_output([exe, 'consts'], text=True)
    return {name: int(v) for name, v in (l.split() for l in out.splitlines())}


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def planned(exe, golden):
    """the program's output in the form of the golden file"""
    forced = []
    for p in golden['plans']:
        pair = (p['late_only'], p['shape'])
        if pair != (-1, -1) and pair not in forced:
            forced.append(pair)
    out = subprocess.check_output(
        [exe, 'plan'] + [str(v) for pair in forced for v in pair], text=True)
    rounds, plans = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == 'rounds':
            rounds[f[1]] = [int(v) for v in f[2:]]
        else:
            key = tuple(int(v) for v in f[1:4])
            plans.setdefault(key, {})[f[0]] = [int(v) for v in f[4:]]
    return {'rounds': rounds,
            'plans': [dict(kt1=k[0], late_only=k[1], shape=k[2], **v)
                      for k, v in plans.items()]}


def records(ints):
    assert len(ints) % 5 == 0
    return [tuple(ints[i:i + 5]) for i in range(0, len(ints), 5)]


def chosen(planned, kt1):
    """jobs and schedule of g_plan(kt1, -1, -1)"""
    p, = [p for p in planned['plans']
          if (p['kt1'], p['late_only'], p['shape']) == (kt1, -1, -1)]
    return records(p['jobs']), p['sched']


def check_jobs(jobs, kt1):
    """coverage and shapes of one job list"""
    cover = [np.zeros(t, dtype=int) for t in layer_tiles(kt1)]
    for layer, kt0, nk, ht0, nh in jobs:
        assert 0 <= layer < 4
        assert (nk, nh) in SHAPES, (kt1, layer, nk, nh)
        kt_n, ht_n = cover[layer].shape
        assert 0 <= kt0 and kt0 + nk <= kt_n, (kt1, layer, kt0, nk)
        assert 0 <= ht0 and ht0 + nh <= ht_n, (kt1, layer, ht0, nh)
        cover[layer][kt0:kt0 + nk, ht0:ht0 + nh] += 1
    assert sum(c.size for c in cover) == 45 + 7 * (kt1 - 1)
    for layer, c in enumerate(cover):
        assert (c == 1).all(), (kt1, layer, c)


@pytest.mark.parametrize('kt1', range(1, 10))
def test_every_tile_has_one_job_of_a_shape_g_job_runs(planned, consts, kt1):
    rounds = records(planned['rounds'][str(kt1)])
    check_jobs(rounds, kt1)
    assert len(rounds) <= 32                 # two rounds of 16 workgroups
    assert 4 * 5 * len(rounds) <= consts['JOBS_SLOT']
    check_jobs(chosen(planned, kt1)[0], kt1)


@pytest.mark.parametrize('kt1', range(1, 10))
def test_schedule(planned, consts, kt1):
    jobs, sched = chosen(planned, kt1)
    assert len(sched) == 2 * consts['XCD_SLOTS']
    early, late = sched[0::2], sched[1::2]
    assert sorted(j for j in early + late if j >= 0) == list(range(len(jobs)))
    # these run FB meanwhile
    assert all(j == -1 for j in early[:consts['G_ROWT']])
    assert all(jobs[j][0] in (1, 2, 3) for j in early if j >= 0)
    assert all(jobs[j][0] == 0 for j in late if j >= 0)
    assert all(j >= -1 for j in sched)
    # [schedule][its job records] in one slot
    assert 4 * (len(sched) + 5 * len(jobs)) <= consts['SCHED_SLOT']


def test_job_counts(planned):
    """the figures of the planner this one was moved from, built on its own"""
    plan = [chosen(planned, kt1) for kt1 in range(1, 10)]
    n_early = [sum(j >= 0 for j in s[0::2]) for _, s in plan]
    n_late = [sum(j >= 0 for j in s[1::2]) for _, s in plan]
    assert [len(j) for j, _ in plan] == [26, 32, 31, 32, 41, 48, 42, 49, 45]
    assert n_early == [19, 18, 19, 18, 19, 19, 19, 19, 19]
    assert n_late == [7, 14, 12, 14, 22, 29, 23, 30, 26]
    assert [len(records(planned['rounds'][str(k)])) for k in range(1, 10)] == \
        [24, 24, 31, 31, 29, 29, 27, 27, 31]


def test_planner_is_the_recorded_one(planned, golden):
    """Bit for bit what the planner gave before it moved to the header, for
    kt1 1 .. 9: unforced, and with (late_only, shape) forced -- then through
    the NB_TRAIN_LATE_ONLY / NB_TRAIN_LATE_SHAPE switches, now through the
    arguments of g_plan (pairs of profiles/r06/train_plan_sweep.txt, and each
    of the two forced alone; a pair no plan exists for gives empty lists)."""
    assert len(golden['plans']) == 9 * 6
    assert sorted(planned['rounds']) == sorted(golden['rounds'])
    assert planned['rounds'] == golden['rounds']
    key = lambda p: (p['kt1'], p['late_only'], p['shape'])
    assert sorted(map(key, planned['plans'])) == \
        sorted(map(key, golden['plans']))
    want = {key(p): p for p in golden['plans']}
    for p in planned['plans']:
        assert p == want[key(p)], key(p)


def tile_index(c, r):
    # element (c, r) of a 16 x 16 tile (nb_train_plan.h, written out again)
    return ((c // 8) * 64 + ((c // 2) % 4) * 16 + r) * 2 + c % 2


@pytest.mark.parametrize('n_dim, kt1', [(1, 1), (15, 1), (16, 2), (50, 4),
                                        (128, 9)])
def test_pack_network(exe, tmp_path, n_dim, kt1):
    subprocess.check_call([exe, 'pack', str(n_dim), str(tmp_path)])
    w, wt, back = (np.fromfile(str(tmp_path / name)) for name in
                   ('w.bin', 'wt.bin', 'back.bin'))
    tiles = layer_tiles(kt1)
    assert w.size == 256 * sum(k * h for k, h in tiles)
    assert wt.size == 256 * sum(k * h for k, h in tiles[1:])
    rows = (n_dim,) + H[:3]
    # weight_value of the program; the bias is row k = rows
    value = [(l + 1) * 100000.0 + 1000.0 * np.arange(rows[l] + 1)[:, None] +
             np.arange(H[l])[None, :] + 0.25 for l in range(4)]
    # unpack(pack(w)) == w: coefficients, then intercepts, layer by layer
    assert np.array_equal(
        back, np.concatenate([v.ravel() for v in value]))
    want, want_t = np.zeros_like(w), np.zeros_like(wt)
    off = off_t = 0
    for l, (kt_n, ht_n) in enumerate(tiles):
        k, h = np.indices(value[l].shape)
        at = ((k >> 4) * ht_n + (h >> 4)) * 256 + tile_index(k & 15, h & 15)
        assert len(np.unique(at)) == at.size and at.max() < 256 * kt_n * ht_n
        want[off + at] = value[l]
        off += 256 * kt_n * ht_n
        if l > 0:
            # tile [h >> 4][k >> 4], element (h & 15, k & 15)
            at = ((h >> 4) * kt_n + (k >> 4)) * 256 + \
                tile_index(h & 15, k & 15)
            assert len(np.unique(at)) == at.size
            want_t[off_t + at] = value[l]
            off_t += 256 * kt_n * ht_n
    # every weight and bias at its place, 0.0 everywhere else
    assert np.array_equal(w, want)
    assert np.array_equal(wt, want_t)


# ---- XCD ownership (plan_xcds) ----------------------------------------------
@pytest.fixture(scope='module')
def xcd_plans(exe):
    """(n, mask, allowed) -> (two_launch, owned, net[XCD][place])"""
    out = np.array(subprocess.check_output([exe, 'xcds'], text=True).split(),
                   dtype=np.int64).reshape(-1, 5 + 16)
    return {(int(r[0]), int(r[1]), bool(r[2])):
            (bool(r[3]), int(r[4]), r[5:].reshape(8, 2).tolist())
            for r in out}


def test_xcd_ownership_rule(xcd_plans, consts):
    """every network count up to one past the resident limit, every set of
    XCDs in use, resident form allowed or not"""
    n_xcd, limit = consts['XCD_COUNT'], consts['MAX_RESIDENT']
    assert (n_xcd, limit) == (8, 16)
    assert sorted(xcd_plans) == [(n, m, a) for n in range(1, limit + 2)
                                 for m in range(1 << n_xcd)
                                 for a in (False, True)]
    for (n, mask, allowed), (two, owned, net) in xcd_plans.items():
        case = (n, mask, allowed)
        free = [x for x in range(n_xcd) if not mask >> x & 1]
        assert two == (n > limit or not allowed or n > 2 * len(free)), case
        places = [v for pair in net for v in pair if v >= 0]
        if two:
            assert places == [] and owned == 0, case
            continue
        assert sorted(places) == list(range(n)), case   # one place each
        used = [x for x in range(n_xcd) if net[x][0] >= 0 or net[x][1] >= 0]
        assert owned & mask == 0, case
        assert owned == sum(1 << x for x in used), case
        assert all(net[x][0] >= 0 for x in used), case  # place 0 first
        assert used == free[:len(used)], case           # the lowest free ones
        assert len(used) == min(n, len(free)), case
        for i in range(n):
            assert net[used[i % len(used)]][i // len(used)] == i, case


def test_xcd_ownership_cases(xcd_plans):
    none = [-1, -1]
    two, owned, net = xcd_plans[4, 0x00, True]
    assert (two, owned) == (False, 0x0f)
    assert net == [[0, -1], [1, -1], [2, -1], [3, -1]] + 4 * [none]
    two, owned, net = xcd_plans[16, 0x00, True]
    assert (two, owned) == (False, 0xff)
    assert net == [[x, 8 + x] for x in range(8)]
    two, owned, net = xcd_plans[9, 0x00, True]
    assert (two, owned) == (False, 0xff)
    assert net == [[0, 8]] + [[x, -1] for x in range(1, 8)]
    two, owned, net = xcd_plans[5, 0x0f, True]
    assert (two, owned) == (False, 0xf0)
    assert net == 4 * [none] + [[0, 4], [1, -1], [2, -1], [3, -1]]
    for mask in (0x0f, 0xf0, 0x55, 0xc3):             # four XCDs free
        assert xcd_plans[9, mask, True] == (True, 0, 8 * [none])
        assert not xcd_plans[8, mask, True][0]
    assert xcd_plans[17, 0x00, True] == (True, 0, 8 * [none])
    assert xcd_plans[1, 0xff, True] == (True, 0, 8 * [none])
    assert xcd_plans[4, 0x00, False] == (True, 0, 8 * [none])


# ---- layout of the block (pool_layout, block_bytes) --------------------------
def test_pool_layout(exe, consts):
    """W, M, V, WT, stash, loss curve and the 32 scalars of a network lie in
    that order without overlap inside per_net doubles, and the block holds
    the pools of all networks behind the small arrays"""
    out = np.array(subprocess.check_output([exe, 'layout'], text=True).split(),
                   dtype=np.int64).reshape(-1, 12)
    assert [(int(r[0]), int(r[1])) for r in out] == \
        [(kt1, m) for kt1 in range(1, 10) for m in (1, 2, 9999, 10000)]
    # units of a stash row: the input block, activations and deltas of the
    # layers 1-3 with their bias unit, the output delta, each padded to 16
    pad16 = lambda u: (u + 15) // 16 * 16
    upper = 2 * sum(pad16(h + 1) for h in H[:3]) + pad16(H[3])
    for kt1, max_iter, w, m, v, wt, stash, curve, scal, per_net, b1, b16 in \
            out.tolist():
        tiles = layer_tiles(kt1)
        n_w = 256 * sum(k * h for k, h in tiles)
        sizes = [n_w, n_w, n_w, 256 * sum(k * h for k, h in tiles[1:]),
                 16 * consts['G_ROWT'] * (16 * kt1 + upper), max_iter, 32]
        at = [w, m, v, wt, stash, curve, scal]
        assert at[0] == 0
        for i in range(7):
            end = at[i + 1] if i < 6 else per_net
            assert at[i] + sizes[i] <= end, (kt1, max_iter, i)
        assert per_net % 512 == 0
        assert per_net - (scal + 32) < 512            # no more than rounding
        assert curve % 2 == 0 and scal % 2 == 0       # 16-byte boundaries
        for n_networks, bytes_ in ((1, b1), (16, b16)):
            need = consts['OFF_POOL'] + 8 * n_networks * per_net
            assert bytes_ % (2 << 20) == 0
            assert need <= bytes_ < need + (2 << 20)


# ---- large stash (stash_choice, large_per_net) -------------------------------
@pytest.mark.parametrize('rows, batch, large, rowt', [
    ((1000,), 200, False, 13), ((1000,), 201, True, 13),
    ((1000,), 209, True, 14), ((1000,), 512, True, 32),
    ((300,), 4096, True, 19), ((50, 5000), 1000, True, 63),
    ((150,), 4096, False, 13)])
def test_stash_choice(exe, consts, rows, batch, large, rowt):
    assert consts['G_ROWT'] == 13 and consts['SMALL_BATCH'] == 200
    for kt1 in (1, 4, 9):
        got = subprocess.check_output(
            [exe, 'stash', str(kt1), str(batch)] + [str(n) for n in rows],
            text=True).split()
        assert (bool(int(got[0])), int(got[1])) == (large, rowt)
        # the stash of rowt row tiles and the loss partial of each
        per_net = int(got[2])
        stash = 16 * rowt * (16 * kt1 + 2 * (112 + 64 + 32) + 16)
        assert per_net % 512 == 0
        assert 0 <= per_net - (stash + rowt) < 512


@pytest.mark.parametrize('rows, batch, want', [
    (1000, 512, (512, 2)), (150, 200, (150, 1)), (1000, 200, (200, 5)),
    (1001, 200, (200, 6)), (1, 200, (1, 1)), (4096, 4096, (4096, 1))])
def test_epoch_steps(exe, rows, batch, want):
    got = subprocess.check_output([exe, 'steps', str(rows), str(batch)],
                                  text=True).split()
    assert tuple(int(v) for v in got) == want
