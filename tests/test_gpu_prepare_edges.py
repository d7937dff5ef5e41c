"""GPU: csrc/voxelize.hip at its edges, against the restatement of tests/_prepare_rule.py.  Every entry of the preparation block of
include/b2m_prepare.h (b2m_vox_shift ... b2m_seg_mode) is called directly through _lib.call / _lib.call_ret on the cases of
tests/_prepare_cases.py -- each of which asserts, when it is built, the predicates that say which edge it reaches, and is shown to
be sharp on the CPU by tests/test_prepare_rule.py -- and then the wrappers of box2mask_amd/prepare.py are held to the rule and to
oracle/prepare_ref.py.  Every comparison is exact (np.array_equal / torch.equal, the shift and the centroids bit for bit); the one
tolerance is the existing rtol 1e-12 between the centroids and numpy's running mean.  No input leaves an entry's contract; refusals
are tested only where the entry or the wrapper checks on the host."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _prepare_cases as C
import _prepare_rule as R

pytestmark = pytest.mark.gpu


def _lib():
    from box2mask_amd import _lib
    return _lib


def _dev(a, dtype, least=0):
    """The array on the device; `least`: allocate at least that many elements (an empty tensor has no address)."""
    a = np.ascontiguousarray(np.asarray(a, dtype))
    if a.size >= least:
        return torch.from_numpy(a).cuda()
    t = torch.zeros(least, dtype=torch.from_numpy(a).dtype, device='cuda')
    return t


def _keys_tensor(keys):
    return _dev(np.array(keys, np.uint64).view(np.int64), np.int64, 1)


def _np(t):
    return t.cpu().numpy()


def _u64(t):
    return [int(k) for k in _np(t).view(np.uint64).tolist()]


def _pow2(n):
    return 1 << max(1, (int(n) - 1).bit_length())


def _filled(shape, value, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device='cuda')


# ----------------------------------------------------------------------------- the unique / sort / rank chain
def _chain(keys, n, n_pad=None, use_async=False):
    """np.unique(return_inverse=True) through b2m_unique_insert[_async], b2m_sort_u64 and b2m_unique_rank, sized as
    box2mask_amd.prepare sizes them (cap = the power of two >= max(2n, 16))."""
    L, ptr = _lib(), _lib().ptr
    cap = _pow2(max(2 * n, 16))
    tkeys, tvals = _filled(cap, 5, torch.int64), _filled(cap, -9, torch.int32)
    slot_of = _filled(max(n, 1), -9, torch.int32)
    ukeys = _filled(max(n_pad or 0, _pow2(max(n, 2))), -1, torch.int64)
    n_unique = _filled(1, -9, torch.int32)
    args = (ptr(keys), n, ptr(tkeys), cap, ptr(slot_of), ptr(ukeys), ptr(n_unique))
    if use_async:
        L.call('b2m_unique_insert_async', *args)
        nu = int(n_unique.item())
    else:
        nu = L.call_ret('b2m_unique_insert', *args)
        assert int(n_unique.item()) == nu
    pad = n_pad or _pow2(max(nu, 2))
    L.call('b2m_sort_u64', ptr(ukeys), pad)
    inverse = _filled(max(n, 1), -9, torch.int64)
    L.call('b2m_unique_rank', ptr(ukeys), nu, ptr(tkeys), ptr(tvals), cap, ptr(slot_of), n, ptr(inverse))
    return SimpleNamespace(n=n, nu=nu, cap=cap, tkeys=tkeys, tvals=tvals, slot_of=slot_of, ukeys=ukeys, pad=pad, inverse=inverse[:n])


def _decode(ch, batch):
    coords = _filled((max(ch.nu, 1), 4), -9, torch.int32)
    _lib().call('b2m_vox_decode', _lib().ptr(ch.ukeys), ch.nu, batch, _lib().ptr(coords))
    return coords[:ch.nu]


def _check_chain(ch, keys_list, uniq, inverse, tag):
    sorted_keys = _u64(ch.ukeys)
    assert ch.nu == len(uniq) and sorted_keys[:ch.nu] == uniq, (tag, 'sorted distinct keys')
    assert all(k == (1 << 64) - 1 for k in sorted_keys[ch.nu:]), (tag, 'the padding stays behind the keys')
    assert np.array_equal(_np(ch.inverse), inverse), (tag, 'inverse')
    table, slot = _u64(ch.tkeys), _np(ch.slot_of)[:ch.n].tolist()
    assert sorted(k for k in table if k != (1 << 64) - 1) == uniq, (tag, 'every distinct key is in the table once')
    assert [table[s] for s in slot] == keys_list, (tag, 'slot_of names the slot of the element\'s key')
    tv = _np(ch.tvals)
    assert [int(tv[s]) for s in slot] == inverse.tolist(), (tag, 'tvals holds the rank')


@pytest.mark.parametrize('name', C.CHAIN_CASES)
def test_unique_sort_rank_decode(name):
    """Both insert variants, twice each: the same distinct keys in the table, the same sorted list, inverse and rows, byte for
    byte.  (Which of two colliding keys takes the first slot of a probe sequence is decided by arrival; the contract promises the
    slot of every element, not a layout, so the tables are compared as key sets and through slot_of.)"""
    c = C.chain_case(name)
    n = len(c.keys)
    if c.tup is not None:
        want = R.unique_tuples(c.tup)
        uniq, inverse = [C.pack(t) for t in want[0]], want[1]
        assert uniq == R.unique_keys(c.keys)[0]                   # (tuple order is the numeric order of the packed key)
    else:
        uniq, inverse = R.unique_keys(c.keys)
    keys = _keys_tensor(c.keys)
    runs = [_chain(keys, n, c.n_pad, use_async=a) for a in (False, True, False, True)]
    for ch in runs:
        assert ch.pad == (c.n_pad or _pow2(max(len(uniq), 2)))
        _check_chain(ch, c.keys, uniq, inverse, name)
        assert torch.equal(ch.ukeys, runs[0].ukeys) and torch.equal(ch.inverse, runs[0].inverse), (name, 'bit identity')
    if c.tup is not None:
        for batch in (0, 7):
            rows = [_np(_decode(ch, batch)) for ch in runs[:2]]
            assert rows[0].tolist() == [[batch] + list(t) for t in want[0]], (name, 'decode', batch)
            assert np.array_equal(rows[0], rows[1])


def test_unique_on_an_empty_input():
    keys = _keys_tensor([])
    for a in (False, True):
        ch = _chain(keys, 0, use_async=a)
        assert ch.nu == 0 and set(_u64(ch.ukeys)) == {(1 << 64) - 1} == set(_u64(ch.tkeys))
        assert _decode(ch, 3).shape == (0, 4)


def test_unique_refuses_a_table_below_2n():
    L, ptr = _lib(), _lib().ptr
    keys = _keys_tensor(list(range(9)))
    tk, sl, uk, nu = _filled(16, 5, torch.int64), _filled(9, -9, torch.int32), _filled(16, -1, torch.int64), _filled(1, -9, torch.int32)
    for cap in (16, 12):                                          # 16 < 2 * 9; 12 is no power of two
        with pytest.raises(L.B2MError):
            L.call_ret('b2m_unique_insert', ptr(keys), 9, ptr(tk), cap, ptr(sl), ptr(uk), ptr(nu))
        with pytest.raises(L.B2MError):
            L.call('b2m_unique_insert_async', ptr(keys), 9, ptr(tk), cap, ptr(sl), ptr(uk), ptr(nu))
    with pytest.raises(L.B2MError):
        L.call('b2m_sort_u64', ptr(uk), 12)
    assert (tk == 5).all() and (sl == -9).all() and (uk == -1).all() and int(nu.item()) == -9


# ----------------------------------------------------------------------------- b2m_vox_shift
def _shift(pos_t, n):
    shift, scratch = _filled(1, 123.0, torch.float64), _filled(1, -9, torch.int64)
    _lib().call('b2m_vox_shift', _lib().ptr(pos_t), n, _lib().ptr(shift), _lib().ptr(scratch))
    return shift


@pytest.mark.parametrize('name', C.SHIFT_CASES)
def test_vox_shift(name):
    c = C.shift_case(name)
    got = _np(_shift(_dev(c.pos, np.float64, 3), len(c.pos)))
    want = np.array([R.shift_of(c.pos)])
    assert got.tobytes() == want.tobytes(), (name, got, want)     # (bytes: -0.0 would compare equal to the +0.0 it must be)


# ----------------------------------------------------------------------------- b2m_vox_keys
def _vox_keys(pos_t, n, shift_t, vs):
    keys, bad = _filled(max(n, 1), -9, torch.int64), _filled(1, 7, torch.int32)
    _lib().call('b2m_vox_keys', _lib().ptr(pos_t), n, _lib().ptr(shift_t), float(vs), _lib().ptr(keys), _lib().ptr(bad))
    return keys, int(bad.item())


@pytest.mark.parametrize('name', C.KEY_CASES)
def test_vox_keys(name):
    c = C.key_case(name)
    n = len(c.pos)
    keys, bad = _vox_keys(_dev(c.pos, np.float64, 3), n, _dev([c.shift], np.float64), c.vs)
    v = R.voxel_index(c.pos, c.shift, c.vs)
    ok = R.in_range(v)
    assert bad == R.bad_count(v), name
    got = _u64(keys)[:n]
    want = iter(R.tuples(v[ok]))
    for i in range(n):
        assert (C.unpack(got[i]) == next(want) and got[i] >> 63 == 0) if ok[i] else got[i] == 0, (name, i)
    if n == 0:
        assert _u64(keys) == [(1 << 64) - 9]                       # nothing written


def test_vox_keys_refuses_a_voxel_size_of_zero():
    L = _lib()
    pos, shift = _dev(np.ones((4, 3)), np.float64), _dev([0.0], np.float64)
    keys, bad = _filled(4, -9, torch.int64), _filled(1, 7, torch.int32)
    for vs in (0.0, -0.5, float('nan')):
        with pytest.raises(L.B2MError):
            L.call('b2m_vox_keys', L.ptr(pos), 4, L.ptr(shift), vs, L.ptr(keys), L.ptr(bad))
    assert (keys == -9).all() and int(bad.item()) == 7


# ----------------------------------------------------------------------------- the entries from points to associated points
def _device_voxels(pos, vs):
    """shift -> keys -> unique chain -> decode -> nearest, entry by entry."""
    L, ptr = _lib(), _lib().ptr
    n = len(pos)
    pos_t = _dev(pos, np.float64, 3)
    shift = _shift(pos_t, n)
    keys, bad = _vox_keys(pos_t, n, shift, vs)
    assert bad == 0
    ch = _chain(keys, n, use_async=True)
    coords = _decode(ch, 0)
    best, p2v = _filled(ch.nu, 5, torch.int64), _filled(ch.nu, -9, torch.int32)
    L.call('b2m_vox_nearest', ptr(pos_t), n, ptr(shift), float(vs), ptr(ch.tkeys), ptr(ch.tvals), ch.cap, ch.nu, ptr(best), ptr(p2v))
    return SimpleNamespace(shift=shift, coords=coords, vox2point=ch.inverse, point2vox=p2v, best=best, chain=ch)


@pytest.mark.parametrize('name', C.NEAREST_CASES)
def test_vox_nearest(name):
    c = C.nearest_case(name)
    d = [_device_voxels(c.pos, c.vs) for _ in range(2)]
    g, r = d[0], c.rule
    assert _np(g.shift).tobytes() == np.array([r['shift']]).tobytes(), name
    assert np.array_equal(_np(g.coords)[:, 1:], r['vox_coords'].astype(np.int32)) and (g.coords[:, 0] == 0).all(), name
    assert np.array_equal(_np(g.vox2point), r['vox2point']), name
    assert np.array_equal(_np(g.point2vox), r['point2vox'].astype(np.int32)), (name, _np(g.point2vox), r['point2vox'])
    assert np.array_equal(_np(g.best).view(np.float64), r['nearest_d']), (name, 'the winning distance, bit for bit')
    for f in ('coords', 'vox2point', 'point2vox', 'best'):
        assert torch.equal(getattr(d[0], f), getattr(d[1], f)), (name, f, 'bit identity')


# ----------------------------------------------------------------------------- b2m_vox_gather
@pytest.mark.parametrize('name', C.GATHER_CASES)
def test_vox_gather(name):
    L, ptr = _lib(), _lib().ptr
    c = C.gather_case(name)
    n = len(c.point2vox)
    p2v, col, nor, seg = _dev(c.point2vox, np.int32), _dev(c.colors, np.float64), _dev(c.normals, np.float64), _dev(c.segments, np.int64)
    for normals in (None, nor):
        for with_seg in (True, False):
            width = 3 if normals is None else 6
            feats, vseg = _filled((n, width), -9.0, torch.float32), _filled(n, -9, torch.int64)
            L.call('b2m_vox_gather', ptr(p2v), n, ptr(col), ptr(normals), ptr(seg) if with_seg else None, ptr(feats),
                   ptr(vseg) if with_seg else None)
            want_f, want_s = R.gather(c.point2vox, c.colors, None if normals is None else c.normals, c.segments)
            assert want_f.shape == (n, width) and _np(feats).tobytes() == want_f.tobytes(), (name, width)
            assert np.array_equal(_np(vseg), want_s) if with_seg else (vseg == -9).all(), (name, with_seg)
    feats, vseg = _filled((n, 6), -9.0, torch.float32), _filled(n, -9, torch.int64)
    for s, v in ((seg, None), (None, vseg)):                       # one of the two without the other: refused
        with pytest.raises(L.B2MError):
            L.call('b2m_vox_gather', ptr(p2v), n, ptr(col), ptr(nor), ptr(s), ptr(feats), ptr(v))
    assert (feats == -9).all() and (vseg == -9).all()


# ----------------------------------------------------------------------------- b2m_seg_centroid
@pytest.mark.parametrize('name', C.CENTROID_CASES)
def test_seg_centroid(name):
    L, ptr = _lib(), _lib().ptr
    c = C.centroid_case(name)
    n = len(c.vox)
    coords = _dev(np.concatenate([np.full((n, 1), 3), c.vox], 1), np.int32, 4)
    s2v, shift = _dev(c.seg2vox, np.int64, 1), _dev([c.shift], np.float64)
    outs = []
    for _ in range(2):
        sums, counts = _filled(max(3 * c.n_seg, 1), -9, torch.int64), _filled(max(c.n_seg, 1), -9, torch.int32)
        out = _filled((max(c.n_seg, 1), 3), -9.0, torch.float64)
        L.call('b2m_seg_centroid', ptr(coords), ptr(s2v), n, c.n_seg, float(c.vs), ptr(shift), ptr(sums), ptr(counts), ptr(out))
        outs.append(_np(out))
    if c.n_seg == 0:
        assert (outs[0] == -9).all()
        return
    want = R.centroids(c.vox, c.seg2vox, c.n_seg, c.vs, c.shift)
    assert outs[0].tobytes() == want.tobytes() == outs[1].tobytes(), name
    assert np.allclose(outs[0], R.centroid_means(c.vox, c.seg2vox, c.n_seg, c.vs, c.shift), rtol=1e-12, atol=1e-12), name
    assert np.array_equal(_np(counts)[:c.n_seg], np.bincount(c.seg2vox, minlength=c.n_seg))


# ----------------------------------------------------------------------------- b2m_box_membership
def _box_membership(pos, lo, hi, vol, fill=-9):
    L, ptr = _lib(), _lib().ptr
    n, nb = len(pos), len(lo)
    out = [_filled(max(n, 1), fill, torch.int32) for _ in range(3)]
    d = [_dev(pos, np.float64, 3), _dev(lo, np.float64), _dev(hi, np.float64), _dev(vol, np.float32)]
    L.call('b2m_box_membership', ptr(d[0]), n, *[ptr(x) if nb else None for x in d[1:]], nb, *[ptr(o) for o in out])
    return [_np(o)[:n] for o in out]


@pytest.mark.parametrize('name', C.BOX_CASES)
def test_box_membership(name):
    c = C.box_case(name)
    got, want = _box_membership(c.pos, c.lo, c.hi, c.volume), R.box_membership(c.pos, c.lo, c.hi, c.volume)
    for g, w, what in zip(got, want, ('count', 'first_bb', 'smallest_bb')):
        assert np.array_equal(g, w), (name, what)


def test_box_membership_refuses_1025_boxes():
    L, ptr = _lib(), _lib().ptr
    lo, hi, vol = _dev(np.full((1025, 3), -1.0), np.float64), _dev(np.ones((1025, 3)), np.float64), _dev(np.ones(1025), np.float32)
    pos = _dev(np.zeros((257, 3)), np.float64)
    out = [_filled(257, 77, torch.int32) for _ in range(3)]
    with pytest.raises(L.B2MError):
        L.call('b2m_box_membership', ptr(pos), 257, ptr(lo), ptr(hi), ptr(vol), 1025, *[ptr(o) for o in out])
    with pytest.raises(L.B2MError):
        L.call('b2m_box_membership', ptr(pos), 257, ptr(lo), ptr(hi), ptr(vol), -1, *[ptr(o) for o in out])
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in out)


# ----------------------------------------------------------------------------- b2m_obb_membership
@pytest.mark.parametrize('name', C.OBB_CASES)
def test_obb_membership(name):
    L, ptr = _lib(), _lib().ptr
    c = C.obb_case(name)
    n, nb = len(c.pos), len(c.centers)
    out = [_filled(n, -9, torch.int32) for _ in range(2)]
    d = [_dev(c.pos, np.float64), _dev(c.centers, np.float64), _dev(c.rot.reshape(-1, 9), np.float64), _dev(c.half, np.float64)]
    L.call('b2m_obb_membership', ptr(d[0]), n, *[ptr(x) if nb else None for x in d[1:]], nb, *[ptr(o) for o in out])
    for g, w, what in zip(out, R.obb_membership(c.pos, c.centers, c.rot, c.half), ('count', 'first_bb')):
        assert np.array_equal(_np(g), w), (name, what)


# ----------------------------------------------------------------------------- b2m_seg_box_vote, b2m_seg_rank, b2m_seg_mode
def _segment_table(useg):
    """The table b2m_unique_rank leaves for the voxel-level segments: built from a shuffled list that repeats every id."""
    rng = np.random.default_rng(len(useg))
    vox_segments = np.array(list(useg) * 3, np.int64)[rng.permutation(3 * len(useg))]
    ch = _chain(_dev(vox_segments, np.int64), len(vox_segments), use_async=True)
    assert _u64(ch.ukeys)[:ch.nu] == list(useg)
    return ch


@pytest.mark.parametrize('name', C.VOTE_CASES)
def test_seg_box_vote(name):
    L, ptr = _lib(), _lib().ptr
    c = C.vote_case(name)
    n, S = len(c.segments), len(c.useg)
    ch = _segment_table(c.useg)
    seg, cnt, first, small = _dev(c.segments, np.int64), _dev(c.count, np.int32), _dev(c.first_bb, np.int32), _dev(c.smallest_bb, np.int32)
    ids = _dev(c.ids, np.int64) if len(c.ids) else None
    for h in (0, 1, 0):
        best, sop = _filled(S, 5, torch.int64), _filled(n, -9, torch.int32)
        per_seg, per_point = _filled(S, -9, torch.int64), _filled(n, -9, torch.int64)
        L.call('b2m_seg_box_vote', ptr(seg), n, ptr(ch.tkeys), ptr(ch.tvals), ch.cap, S, ptr(cnt), ptr(first), ptr(small), ptr(ids), h,
               ptr(best), ptr(sop), ptr(per_seg), ptr(per_point))
        want = R.segment_vote(c.segments, c.useg, c.count, c.first_bb, c.smallest_bb, c.ids, h)
        for g, w, what in zip((per_point, per_seg, sop), want, ('inst_per_point', 'inst_per_seg', 'seg_of_point')):
            assert np.array_equal(_np(g), w), (name, h, what)


@pytest.mark.parametrize('name', C.RANK_CASES)
def test_seg_rank(name):
    L, ptr = _lib(), _lib().ptr
    c = C.rank_case(name)
    ch = _segment_table(c.useg)
    seg, out = _dev(c.segments, np.int64), _filled(len(c.segments), -9, torch.int32)
    L.call('b2m_seg_rank', ptr(seg), len(c.segments), ptr(ch.tkeys), ptr(ch.tvals), ch.cap, ptr(out))
    assert np.array_equal(_np(out), R.segment_rank(c.segments, c.useg)), name


@pytest.mark.parametrize('name', C.MODE_CASES)
def test_seg_mode(name):
    L, ptr = _lib(), _lib().ptr
    c = C.mode_case(name)
    sop, cls = _dev(c.seg_of_point, np.int32), _dev(c.cls, np.int32)
    hist, mode = _filled(max(c.n_seg * c.n_class, 1), -9, torch.int32), _filled(max(c.n_seg, 1), -9, torch.int32)
    L.call('b2m_seg_mode', ptr(sop), ptr(cls), len(c.cls), c.n_seg, c.n_class, ptr(hist), ptr(mode))
    if c.n_seg == 0:
        assert (hist == -9).all() and (mode == -9).all()
        return
    assert np.array_equal(_np(mode), R.segment_mode(c.seg_of_point, c.cls, c.n_seg, c.n_class)), name
    with pytest.raises(L.B2MError):
        L.call('b2m_seg_mode', ptr(sop), ptr(cls), len(c.cls), c.n_seg, 0, ptr(hist), ptr(mode))


# ----------------------------------------------------------------------------- the wrappers
_ITEM_KEYS = ('vox2point', 'point2vox', 'vox_segments', 'seg2vox', 'seg2point', 'pred2point', 'unique_vox_segments')


def _check_item(item, r, vs, normals=True, pooling=True, tag=''):
    from box2mask_amd import prepare
    assert _np(item['voxel_shift']).tobytes() == np.array([r['shift']]).tobytes(), tag
    assert np.array_equal(_np(item['vox_coords'])[:, 1:], r['vox_coords'].astype(np.int32)) and (item['vox_coords'][:, 0] == 0).all(), tag
    for k in _ITEM_KEYS:
        if not pooling and k in ('seg2vox', 'seg2point'):
            assert k not in item
            continue
        want = r['vox2point'] if (k == 'pred2point' and not pooling) else r['seg2point' if k == 'pred2point' else k]
        got = _np(item[k])
        assert got.dtype == np.int64 and np.array_equal(got, want), (tag, k)
    feats = r['vox_features'] if normals else r['vox_features'][:, :3]
    assert _np(item['vox_features']).tobytes() == np.ascontiguousarray(feats).tobytes(), (tag, 'features')
    assert _np(prepare.vox_world_coords(item)).tobytes() == r['vox_world_coords'].tobytes(), tag
    loc = _np(item['input_location'])
    if pooling:
        assert loc.tobytes() == r['input_location'].tobytes(), (tag, 'centroids, bit for bit against the integer form')
        assert np.allclose(loc, r['input_location_mean'], rtol=1e-12, atol=1e-12), (tag, 'centroids against numpy\'s mean')
    else:
        assert loc.tobytes() == r['vox_world_coords'].tobytes(), tag


@pytest.mark.parametrize('name', C.SCENE_CASES)
def test_voxelize_scene(name):
    from box2mask_amd import prepare
    c = C.scene_case(name)
    _check_item(prepare.voxelize_scene(c.scene, c.vs), c.rule, c.vs, tag=name)
    _check_item(prepare.voxelize_scene(c.scene, c.vs, use_normals_input=False), c.rule, c.vs, normals=False, tag=name + ' no normals')
    _check_item(prepare.voxelize_scene(c.scene, c.vs, do_segment_pooling=False), c.rule, c.vs, pooling=False, tag=name + ' no pooling')


def _same_items(a, b, tag):
    assert set(a) == set(b)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert v.dtype == b[k].dtype and torch.equal(v, b[k]), (tag, k)


def test_scenes_together_equal_one_by_one_and_twice():
    from box2mask_amd import prepare
    cases = [C.scene_case(n) for n in ('one_point', 'ties', 'one_segment')]
    assert len({c.vs for c in cases}) == 1
    together = prepare.voxelize_scenes([c.scene for c in cases], cases[0].vs)
    again = prepare.voxelize_scenes([c.scene for c in cases], cases[0].vs)
    for c, it, it2 in zip(cases, together, again):
        _check_item(it, c.rule, c.vs, tag=c.name)
        _same_items(prepare.voxelize_scene(c.scene, c.vs), it, c.name)
        _same_items(it, it2, c.name + ' (bit identity)')


def test_refused_scenes():
    from box2mask_amd import prepare
    sc = C.scene_case('ties').scene
    empty = {k: v[:0] for k, v in sc.items() if k != 'name'}
    negative = dict(sc, segments=np.where(np.arange(len(sc['segments'])) == 7, -1, sc['segments']))
    nan = dict(sc, positions=np.where(np.arange(len(sc['positions']))[:, None] == 9, np.nan, sc['positions']))
    for bad in (empty, negative, nan):
        with pytest.raises(ValueError):
            prepare.voxelize_scene(bad, 0.5)
        with pytest.raises(ValueError):
            prepare.voxelize_scenes([sc, bad], 0.5)


def test_collate_against_the_rule():
    from box2mask_amd import prepare
    cases = [C.scene_case(n) for n in ('ties', 'one_segment', 'own_segments')]
    items = prepare.voxelize_scenes([c.scene for c in cases], 0.5)
    b = prepare.collate(items, 'test')
    rules = [c.rule for c in cases]
    assert np.array_equal(_np(b['pooling_ids']), R.pooling_ids([r['vox_segments'] for r in rules]))
    assert np.array_equal(_np(b['batch_ids']), np.concatenate([np.full(len(r['unique_vox_segments']), i) for i, r in enumerate(rules)]))
    want = np.concatenate([np.concatenate([np.full((len(r['vox_coords']), 1), i), r['vox_coords']], 1) for i, r in enumerate(rules)])
    assert b['vox_coords'].dtype == torch.int32 and np.array_equal(_np(b['vox_coords']), want)
    assert _np(b['vox_features']).tobytes() == np.concatenate([r['vox_features'] for r in rules]).tobytes()
    assert _np(b['input_location']).tobytes() == np.concatenate([r['input_location'] for r in rules]).astype(np.float32).tobytes()
    assert (items[1]['vox_coords'][:, 0] == 0).all()              # collate works on copies


@pytest.mark.parametrize('kind', C.LABELLED)
def test_associations_against_the_oracle(kind):
    """approx_association / box_supervision of the three datasets on a hand-built scene, under every option, against
    oracle/prepare_ref.py and against the rule."""
    from box2mask_amd import prepare
    from oracle import prepare_ref as O
    c = C.labelled_scene(kind)
    sc, lab = c.scene, c.scene['labels']
    pos, seg, useg = sc['positions'], sc['segments'], c.rule['unique_vox_segments']
    item = prepare.voxelize_scene(sc, c.vs)
    _check_item(item, c.rule, c.vs, tag=kind)

    def same(got, wants, tag):
        for want in wants:
            assert len(got) == len(want), tag
            for g, w in zip(got, want):
                assert (g is None and w is None) or np.array_equal(_np(g), w), (kind, tag)

    for h in (False, True):
        cfg = SimpleNamespace(smallest_bb_heuristic=h)
        same(prepare.approx_association(item, lab, cfg), (O.approx_association(pos, seg, lab, useg, h),
                                                          R.scannet_association(pos, seg, lab, useg, h)), ('scannet segment', h))
        it = prepare.box_supervision(prepare.voxelize_scene(sc, c.vs), lab, cfg)
        ips = O.approx_association(pos, seg, lab, useg, h)[1]
        gt = O.bbs_supervision(c.rule, lab, ips)
        assert np.array_equal(_np(it['pseudo_inst'][1]), ips)
        for k in ('fg_instances', 'gt_semantics', 'gt_bb_bounds'):
            assert np.array_equal(_np(it[k]), gt[k]), (kind, k, h)
        assert np.array_equal(_np(it['gt_bb_offsets']), gt['gt_bb_offsets']), (kind, 'offsets', h)
        for how, mv in (('majority', True), ('point', False)):
            cfg = SimpleNamespace(smallest_bb_heuristic=h, majority_vote=mv, point_association=not mv)
            same(prepare.approx_association(item, lab, cfg), (O.approx_association_points(pos, seg, lab, useg, h, mv),
                                                              R.scannet_association(pos, seg, lab, useg, h, how)), ('scannet', how, h))
    for pa in (False, True):
        cfg = SimpleNamespace(point_association=pa)
        same(prepare.approx_association(item, lab, cfg, 'arkitscenes'), (O.arkit_association(pos, seg, lab, useg, pa),
                                                                         R.arkit_association(pos, seg, lab, useg, pa)), ('arkit', pa))
        for ign in (False, True):
            cfg = SimpleNamespace(point_association=pa, ignore_wall_ceiling_floor=ign)
            same(prepare.approx_association(item, lab, cfg, 's3dis'), (O.s3dis_association(pos, seg, lab, useg, pa, ign),
                                                                       R.s3dis_association(pos, seg, lab, useg, pa, ign)), ('s3dis', pa, ign))
    it = prepare.box_supervision(prepare.voxelize_scene(sc, c.vs), lab, SimpleNamespace(point_association=False), 'arkitscenes')
    assert np.array_equal(_np(it['pseudo_inst'][1]), O.arkit_association(pos, seg, lab, useg, False)[1])
    for ign in (False, True):
        it = prepare.box_supervision(prepare.voxelize_scene(sc, c.vs), lab, SimpleNamespace(ignore_wall_ceiling_floor=ign), 's3dis')
        want = O.s3dis_association(pos, seg, lab, useg, False, ign)
        assert np.array_equal(_np(it['pseudo_inst'][1]), want[2]) and np.array_equal(_np(it['gt_per_vox_semantics']), want[1][c.rule['point2vox']])
