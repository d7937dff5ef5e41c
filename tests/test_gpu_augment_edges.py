"""GPU: csrc/augment.hip at its edges, bit for bit against the restatement of tests/_augment_rule.py.  Every entry of the augmentation
block of include/b2m_prepare.h is called DIRECTLY through _lib.call on the cases of tests/_augment_cases.py -- each of which asserts,
when it is built, the predicates that say which edge it reaches, and is shown to have teeth on the CPU by tests/test_augment_rule.py.

Every array an entry writes sits inside poisoned padding, so "writes only its outputs" is checked with every call.  Every comparison
is on the raw bits (NaN positions equal); the one exception is the sign of a zero box centre in the case 'signed_zero', compared
with ==.  Refusals are tested where the entry checks on the host: the outputs keep their poison."""
import numpy as np
import pytest
import torch

import _augment_cases as C
import _augment_rule as R

pytestmark = pytest.mark.gpu

PAD = 64
POISON = {torch.float64: -777.25, torch.float32: -777.25, torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a}


def _L():
    from box2mask_amd import _lib
    return _lib


class Out:
    """An array an entry writes (or updates in place), inside PAD poisoned elements on either side."""

    def __init__(self, init=None, shape=None, dtype=torch.float64):
        if init is not None:
            init = torch.from_numpy(np.array(init, order='C'))
            shape, dtype = tuple(init.shape), init.dtype
        self.n = int(np.prod(shape))
        self.shape = shape
        self.poison = POISON[dtype]
        self.full = torch.full((self.n + 2 * PAD,), self.poison, dtype=dtype, device='cuda')
        if init is not None:
            self.full[PAD:PAD + self.n] = init.reshape(-1).cuda()
        self.ptr = self.full[PAD:].data_ptr()

    def get(self):
        """The array, after checking that the padding still holds its poison."""
        f = self.full.cpu()
        assert bool((f[:PAD] == self.poison).all()) and bool((f[PAD + self.n:] == self.poison).all()), 'written outside the output'
        return f[PAD:PAD + self.n].reshape(self.shape).numpy()

    def untouched(self):
        return bool((self.full == self.poison).all())


def _dev(a, dtype=None):
    a = np.array(a, dtype=dtype, order='C')
    return torch.from_numpy(a).cuda()


def _host(a):
    """A host array and its address: what the *_host arguments read during the call."""
    import ctypes
    a = np.array(a, np.float64, order='C')
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want, tag):
    assert got.dtype == np.asarray(want).dtype and got.shape == np.asarray(want).shape, (tag, got.dtype, got.shape)
    if not R.same_bits(got, want):
        bad = np.nonzero(np.atleast_1d((R.bits(got) != R.bits(np.ascontiguousarray(want))).reshape(-1)))[0]
        raise AssertionError('%s: %d of %d elements differ in their bits; first at %s: got %r want %r'
                             % (tag, len(bad), got.size, bad[:4], got.reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]]))


# ----------------------------------------------------------------------------- b2m_aug_stats
def _stats(x_t, n):
    partial, stats = Out(shape=(256 * 12,)), Out(shape=(12,))
    _L().call('b2m_aug_stats', x_t.data_ptr(), n, partial.ptr, stats.ptr)
    partial.get()
    return stats.get()


@pytest.mark.parametrize('name', C.STATS_CASES)
def test_stats(name):
    c = C.stats_case(name)
    x = _dev(c.x)
    got = _stats(x, len(c.x))
    _same(got, R.stats(c.x)[0], name)
    if name == C.STATS_LARGEST:
        _same(_stats(x, len(c.x)), got, name + ' (second run)')


def test_stats_refusals():
    L = _L()
    x = _dev(np.ones((4, 3)))
    partial, stats = Out(shape=(256 * 12,)), Out(shape=(12,))
    for args in ((x.data_ptr(), 0, partial.ptr, stats.ptr), (None, 4, partial.ptr, stats.ptr), (x.data_ptr(), 4, None, stats.ptr),
                 (x.data_ptr(), 4, partial.ptr, None), (x.data_ptr(), 1 << 31, partial.ptr, stats.ptr)):
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_stats', *args)
    torch.cuda.synchronize()
    assert partial.untouched() and stats.untouched()


# ----------------------------------------------------------------------------- b2m_aug_affine
def _affine(c):
    """The entry on a case; a device centre comes from b2m_aug_stats itself (and the rule is fed the rule's)."""
    L = _L()
    n = len(c.pos)
    pos, nrm = Out(c.pos), (Out(c.normals) if c.normals is not None else None)
    m, mp = _host(c.M.reshape(9))
    c_host = c_dev = None
    keep = []
    if c.centre is not None and c.centre[0] == 'host':
        keep.append(_host(c.centre[1]))
        c_host = keep[-1][1]
    elif c.centre is not None:
        st = _dev(_stats(_dev(c.pos), n))
        keep.append(st)
        c_dev = (st[0:3] if c.centre[0] == 'mean' else st[3:6]).data_ptr()
    t = None
    if c.t is not None:
        keep.append(_host(c.t))
        t = keep[-1][1]
    L.call('b2m_aug_affine', pos.ptr, nrm.ptr if nrm else None, n, mp, c_host, c_dev, t, 1 if c.recentre else 0)
    return pos.get(), (nrm.get() if nrm else None)


@pytest.mark.parametrize('name', C.AFFINE_CASES)
def test_affine(name):
    c = C.affine_case(name)
    got_p, got_n = _affine(c)
    want_p, want_n = R.affine(c.pos, c.normals, c.M, C.affine_centre(c), c.t, c.recentre)
    _same(got_p, want_p, name + ' positions')
    assert (got_n is None) == (want_n is None)
    if got_n is not None:
        _same(got_n, want_n, name + ' normals')
    if name == C.AFFINE_LARGEST:
        again = _affine(c)
        _same(again[0], got_p, name + ' (second run)')
        _same(again[1], got_n, name + ' (second run)')


def test_affine_refusals():
    L = _L()
    pos = Out(np.ones((4, 3)))
    m, mp = _host(np.eye(3).reshape(9))
    for args in ((pos.ptr, None, 0, mp, None, None, None, 1), (None, None, 4, mp, None, None, None, 1),
                 (pos.ptr, None, 4, None, None, None, None, 1)):
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_affine', *args)
    torch.cuda.synchronize()
    assert np.array_equal(pos.get(), np.ones((4, 3)))


# ----------------------------------------------------------------------------- b2m_aug_axpy
@pytest.mark.parametrize('name', C.AXPY_CASES)
def test_axpy(name):
    L = _L()
    c = C.axpy_case(name)
    runs = []
    for _ in range(2):
        x = Out(c.x)
        y = _dev(c.y)
        L.call('b2m_aug_axpy', x.ptr, y.data_ptr(), float(c.a), len(c.x))
        runs.append(x.get())
    _same(runs[0], R.axpy(c.x, c.y, c.a), name)
    _same(runs[1], runs[0], name + ' (second run)')
    x = Out(c.x)
    for args in ((x.ptr, None, 1.0, len(c.x)), (None, x.ptr, 1.0, len(c.x)), (x.ptr, x.ptr, 1.0, 0)):
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_axpy', *args)
    torch.cuda.synchronize()
    _same(x.get(), np.asarray(c.x), name + ' (refused calls write nothing)')


# ----------------------------------------------------------------------------- b2m_aug_blur
def _blur(grid):
    g, tmp = Out(grid), Out(shape=grid.shape, dtype=torch.float32)
    _L().call('b2m_aug_blur', g.ptr, tmp.ptr, *grid.shape[:3])
    tmp.get()
    return g.get()


@pytest.mark.parametrize('name', C.BLUR_CASES)
def test_blur(name):
    c = C.blur_case(name)
    got = _blur(c.grid)
    _same(got, R.blur(c.grid), name)
    if name == C.BLUR_LARGEST:
        _same(_blur(c.grid), got, name + ' (second run)')


def test_blur_refusals():
    """An axis of one node, NULLs, and 1024^3 nodes -- refused on the arguments alone: nothing of that size is allocated."""
    L = _L()
    g, tmp = Out(shape=(8,), dtype=torch.float32), Out(shape=(8,), dtype=torch.float32)
    for dims in C.BLUR_REFUSED:
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_blur', g.ptr, tmp.ptr, *dims)
    for a, b in ((None, tmp.ptr), (g.ptr, None)):
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_blur', a, b, 2, 2, 2)
    torch.cuda.synchronize()
    assert g.untouched() and tmp.untouched()


# ----------------------------------------------------------------------------- b2m_aug_displace
def _displace(c):
    pos = Out(c.pos)
    keep = [_host(v) for v in (c.lo, c.step, c.hi)]
    grid = _dev(c.grid)
    _L().call('b2m_aug_displace', pos.ptr, len(c.pos), grid.data_ptr(), *[int(v) for v in c.n], *[k[1] for k in keep],
              float(c.magnitude))
    return pos.get()


@pytest.mark.parametrize('name', C.DISPLACE_CASES)
def test_displace(name):
    c = C.displace_case(name)
    got = _displace(c)
    want, branch = R.displace(c.pos, c.grid, c.lo, c.step, c.hi, c.n, c.magnitude)
    _same(got, want, name)
    outside = ~((c.pos >= c.lo) & (c.pos <= c.hi)).all(1)
    _same(got[outside], np.asarray(c.pos)[outside], name + ' (outside, NaN and infinite points keep their bits)')
    if name == C.DISPLACE_LARGEST:
        _same(_displace(c), got, name + ' (second run)')


def test_displace_refusals():
    L = _L()
    pos = Out(np.ones((5, 3)))
    grid = _dev(np.zeros((3, 3, 3, 3), np.float32))
    for what, (n, dims, lo, step, hi) in C.DISPLACE_REFUSED.items():
        keep = [_host(v) for v in (lo, step, hi)]
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_displace', pos.ptr, n, grid.data_ptr(), *dims, *[k[1] for k in keep], 1.0)
    keep = [_host(v) for v in ((0.0,) * 3, (1.0,) * 3, (2.0,) * 3)]
    ok = [pos.ptr, 5, grid.data_ptr(), 3, 3, 3, keep[0][1], keep[1][1], keep[2][1], 1.0]
    for k in (0, 2, 6, 7, 8):
        args = list(ok)
        args[k] = None
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_displace', *args)
    torch.cuda.synchronize()
    assert np.array_equal(pos.get(), np.ones((5, 3)))


# ----------------------------------------------------------------------------- b2m_aug_vertex_normals
def _normals(c):
    V = len(c.pos)
    out = Out(shape=(V, 3))
    faces = _dev(c.faces) if c.faces is not None else None
    face_of = _dev(c.face_of) if c.face_of is not None else None
    pos, row_ptr = _dev(c.pos), _dev(c.row_ptr)                             # (every input stays referenced until the call is made)
    _L().call('b2m_aug_vertex_normals', pos.data_ptr(), V, faces.data_ptr() if faces is not None else None,
              0 if c.faces is None else len(c.faces), row_ptr.data_ptr(), face_of.data_ptr() if face_of is not None else None,
              out.ptr)
    return out.get()


@pytest.mark.parametrize('name', C.NORMALS_CASES)
def test_vertex_normals(name):
    c = C.normals_case(name)
    got = _normals(c)
    _same(got, R.vertex_normals(c.pos, c.faces, c.row_ptr, c.face_of), name)
    if name == C.NORMALS_LARGEST:
        _same(_normals(c), got, name + ' (second run)')
    if c.faces is not None and name != 'bad_values':                       # the product's own CSR is the rule's
        from box2mask_amd import augment
        rp, fo = augment.vertex_face_csr(_dev(c.faces), len(c.pos))
        assert np.array_equal(rp.cpu().numpy(), c.row_ptr) and np.array_equal(fo.cpu().numpy(), c.face_of)


def test_vertex_normals_refusals():
    L = _L()
    c = C.normals_case('isolated')
    pos, faces, rp, fo = _dev(c.pos), _dev(c.faces), _dev(c.row_ptr), _dev(c.face_of)
    out = Out(shape=(40, 3))
    ok = [pos.data_ptr(), 40, faces.data_ptr(), 60, rp.data_ptr(), fo.data_ptr(), out.ptr]
    for k, v in ((0, None), (1, 0), (2, None), (3, -1), (4, None), (5, None), (6, None)):
        args = list(ok)
        args[k] = v
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_vertex_normals', *args)
    torch.cuda.synchronize()
    assert out.untouched()


# ----------------------------------------------------------------------------- b2m_aug_colour
def _colour(c, stats12):
    col = Out(c.col)
    keep = _host(c.tr)
    st, jit = _dev(stats12), _dev(c.jitter)
    _L().call('b2m_aug_colour', col.ptr, len(c.col), st.data_ptr(), int(c.flags), float(c.blend), keep[1], jit.data_ptr())
    return col.get()


@pytest.mark.parametrize('name', C.COLOUR_CASES)
def test_colour(name):
    c = C.colour_case(name)
    st = R.stats(c.col)[0]
    got = _colour(c, st)
    _same(got, R.colour(c.col, st, c.flags, c.blend, c.tr, c.jitter), name)
    if c.flags & 1:                                                        # the device's own statistics are the same bits
        _same(_stats(_dev(c.col), len(c.col)), st, name + ' statistics')
    if name == C.COLOUR_LARGEST:
        _same(_colour(c, st), got, name + ' (second run)')


def test_colour_refusals():
    L = _L()
    c = C.colour_case('n:85')
    col = Out(c.col)
    st, jit = _dev(R.stats(c.col)[0]), _dev(c.jitter)
    tr = _host(c.tr)
    bad = [(col.ptr, 85, st.data_ptr(), -1, 0.5, tr[1], jit.data_ptr()), (col.ptr, 85, st.data_ptr(), 8, 0.5, tr[1], jit.data_ptr()),
           (col.ptr, 85, None, 1, 0.5, tr[1], jit.data_ptr()), (col.ptr, 85, st.data_ptr(), 2, 0.5, None, jit.data_ptr()),
           (col.ptr, 85, st.data_ptr(), 4, 0.5, tr[1], None), (col.ptr, 85, None, 7, 0.5, tr[1], jit.data_ptr()),
           (None, 85, st.data_ptr(), 7, 0.5, tr[1], jit.data_ptr()), (col.ptr, 0, st.data_ptr(), 7, 0.5, tr[1], jit.data_ptr())]
    for args in bad:
        with pytest.raises(L.B2MError):
            L.call('b2m_aug_colour', *args)
    torch.cuda.synchronize()
    _same(col.get(), np.asarray(c.col), 'refused calls write nothing')
    L.call('b2m_aug_colour', col.ptr, 85, None, 0, 0.5, None, None)          # no flag: no array is needed, nothing changes
    _same(col.get(), np.asarray(c.col), 'flags 0')


# ----------------------------------------------------------------------------- b2m_inst_boxes
_BOX_OUT = (('centers64', 3, torch.float64), ('per_sem', 1, torch.int32), ('per_centers', 3, torch.float32), ('per_bounds', 3, torch.float32),
            ('per_radius', 1, torch.float32))


def _boxes(c):
    P, I = len(c.pos), c.n_inst
    o = {k: Out(shape=(I, w) if w > 1 else (I,), dtype=dt) for k, w, dt in _BOX_OUT}
    o['offsets'], o['distances'] = Out(shape=(P, 3), dtype=torch.float32), Out(shape=(P,), dtype=torch.float32)
    o['missing'], o['acc'] = Out(shape=(1,), dtype=torch.int32), Out(shape=(8 * I,), dtype=torch.int64)
    pos, inst, sem = _dev(c.pos), _dev(c.inst), _dev(c.sem)
    _L().call('b2m_inst_boxes', pos.data_ptr(), inst.data_ptr(), sem.data_ptr(), P, I, o['acc'].ptr,
              o['centers64'].ptr, o['per_sem'].ptr, o['per_centers'].ptr, o['per_bounds'].ptr, o['per_radius'].ptr, o['offsets'].ptr,
              o['distances'].ptr, o['missing'].ptr)
    return {k: v.get() for k, v in o.items()}


@pytest.mark.parametrize('name', C.BOX_CASES)
def test_inst_boxes(name):
    c = C.box_case(name)
    got = _boxes(c)
    want = R.inst_boxes(c.pos, c.inst, c.sem, c.n_inst)
    assert int(got['missing'][0]) == want['missing'], name
    for k in ('centers64', 'per_sem', 'per_centers', 'per_bounds', 'per_radius', 'offsets', 'distances'):
        if name == 'signed_zero' and k in ('centers64', 'per_centers'):
            # the sign of a zero centre depends on an order the contract does not fix
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
        else:
            _same(got[k], want[k], '%s %s' % (name, k))
    if name == 'missing3':
        assert int(got['missing'][0]) == 3
        for k in ('centers64', 'per_sem', 'per_centers', 'per_bounds', 'per_radius'):
            assert not got[k][[0, 17, 39]].any(), (name, k)
    if name == 'out_of_range':
        bad = (c.inst < 0) | (c.inst >= c.n_inst)
        assert bad.sum() == 5 and not got['offsets'][bad].any() and not got['distances'][bad].any()
    if name == C.BOX_LARGEST:
        again = _boxes(c)
        for k in got:
            if k != 'acc':
                _same(again[k], got[k], '%s %s (second run)' % (name, k))


@pytest.mark.parametrize('name', C.BOX_DENSE)
def test_instance_labels(name):
    """The wrapper on the same cases: the gathered per-point arrays included."""
    from box2mask_amd import augment
    c = C.box_case(name)
    w = R.inst_boxes(c.pos, c.inst, c.sem, c.n_inst)
    seg2inst = np.arange(3)
    lab = augment.instance_labels({'positions': np.array(c.pos)}, np.array(c.sem), np.array(c.inst), seg2inst)
    want = {'bb_centers': w['per_centers'][c.inst], 'bb_offsets': w['offsets'], 'bb_bounds': w['per_bounds'][c.inst],
            'bb_center_distances': w['distances'][:, None], 'bb_radius': w['per_radius'][c.inst][:, None],
            'unique_instances': np.arange(c.n_inst, dtype=np.int64), 'per_instance_semantics': w['per_sem'],
            'per_instance_bb_centers': w['per_centers'], 'per_instance_bb_bounds': w['per_bounds'], 'per_instance_bb_radius': w['per_radius'],
            'semantics': np.asarray(c.sem), 'instances': np.asarray(c.inst)}
    for k, v in want.items():
        got = lab[k].cpu().numpy()
        if name == 'signed_zero' and k in ('bb_centers', 'per_instance_bb_centers'):
            assert got.dtype == v.dtype and np.array_equal(got, v), (name, k)
        else:
            _same(got, v, '%s %s' % (name, k))
    assert lab['seg2inst'] is seg2inst


def test_instance_labels_refuses_what_is_not_dense():
    from box2mask_amd import augment
    for name in ('missing3', 'out_of_range'):
        c = C.box_case(name)
        with pytest.raises(ValueError, match='dense'):
            augment.instance_labels({'positions': np.array(c.pos)}, np.array(c.sem), np.array(c.inst), None)


def test_inst_boxes_refusals():
    L = _L()
    c = C.box_case('one_point')
    P, I = len(c.pos), c.n_inst
    pos, inst, sem = _dev(c.pos), _dev(c.inst), _dev(c.sem)
    outs = [Out(shape=(8 * I,), dtype=torch.int64), Out(shape=(I, 3)), Out(shape=(I,), dtype=torch.int32),
            Out(shape=(I, 3), dtype=torch.float32), Out(shape=(I, 3), dtype=torch.float32), Out(shape=(I,), dtype=torch.float32),
            Out(shape=(P, 3), dtype=torch.float32), Out(shape=(P,), dtype=torch.float32), Out(shape=(1,), dtype=torch.int32)]
    ok = [pos.data_ptr(), inst.data_ptr(), sem.data_ptr(), P, I] + [o.ptr for o in outs]
    changes = [(3, 0), (4, 0), (4, P + 1), (3, 1 << 31)] + [(k, None) for k in (0, 1, 2)] + [(5 + k, None) for k in range(len(outs))]
    for k, v in changes:
        args = list(ok)
        args[k] = v
        with pytest.raises(L.B2MError):
            L.call('b2m_inst_boxes', *args)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
