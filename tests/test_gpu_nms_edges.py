"""GPU: csrc/nms.hip at its edges, bit for bit against the rule of tests/_nms_rule.py -- box counts around the search window, the
bitmap word and the LDS / global sort threshold, hand-built visiting orders that make the search skip whole windows, score ties,
the two zeros, infinite scores, an IoU exactly at the threshold, degenerate and non-finite boxes, max_k below / at the cluster
count, the documented ceiling and the refusals beyond it, the batch forms with empty scenes; projection, mask NMS, the label and
instance histograms, the gathers and set_ious at every stride and chunk size of their kernels.  The cases and the predicates
that say which branch each one reaches live in _nms_rule.py and are shown to be sharp on the CPU by tests/test_nms_rule.py.
Every comparison is exact (floats by their bit pattern, a NaN equal to any NaN); outputs are pre-filled with sentinels wherever
"not written" is part of the contract."""
import numpy as np
import pytest
import torch

import _nms_rule as R

pytestmark = pytest.mark.gpu
F = np.float32
SENT_W = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _np(t):
    return t.cpu().numpy()


def _full(shape, value, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device='cuda')


def _addr(devs):
    def address(s, name):
        t = devs[s].get(name)
        return 0 if t is None or t.numel() == 0 else t.data_ptr()
    return address


def _table(scenes, devs):
    return torch.from_numpy(R.mask_desc(scenes, _addr(devs)).reshape(-1)).cuda()


# ----------------------------------------------------------------------------- clustering
def _nmc_buffers(n, heat_rows):
    heat = _dev(np.full((heat_rows, n), R.SENT_F, F)) if heat_rows else None
    return dict(reps=_full(n, R.SENT_I, torch.int32), assign=_full(n, R.SENT_I, torch.int32), heat=heat,
                k=_full(1, R.SENT_I, torch.int32), order=_full(R.npow2(n), -1, torch.int64))


def _call_nmc(boxes_dev, n, th, max_k, o):
    from box2mask_amd import _lib
    _lib.call('b2m_nmc', boxes_dev.data_ptr(), n, float(th), max_k, o['reps'].data_ptr(), o['assign'].data_ptr(),
              None if o['heat'] is None else o['heat'].data_ptr(), o['k'].data_ptr(), o['order'].data_ptr())


def _assert_nmc(got, want, n, tag):
    k = int(got['k'].item())
    assert k == want['k'], (tag, k, want['k'])
    reps = _np(got['reps'])
    assert np.array_equal(reps[:k], want['reps']) and (reps[k:] == R.SENT_I).all(), (tag, 'reps')
    assert np.array_equal(_np(got['order'])[:n] & 0xFFFFFFFF, want['order']), (tag, 'order')
    assert np.array_equal(_np(got['assign']), want['assign']), (tag, 'assign')
    if got['heat'] is not None:
        assert R.same_floats(_np(got['heat']), want['heat']), (tag, 'heat')            # sentinel rows included


def _check_nmc_direct(c):
    n = len(c.boxes)
    o = _nmc_buffers(n, c.heat_rows)
    _call_nmc(_dev(c.boxes), n, c.th, c.max_k, o)
    want = R.nmc(c.boxes, c.th, c.max_k, c.heat_rows)
    _assert_nmc(o, want, n, c.name)
    return want


def _check_nmc_wrapper(c):
    """NMS_clustering: representatives, heat-maps, and the clusters it derives from `order` and `assign`."""
    from box2mask_amd import iou_nms
    want = R.nmc(c.boxes, c.th, len(c.boxes))
    reps, clusters, heat = iou_nms.NMS_clustering(torch.from_numpy(c.boxes), float(c.th))
    assert reps.dtype == torch.int64 and np.array_equal(reps.numpy(), want['reps']), c.name
    assert R.same_floats(heat.numpy(), want['heat'][:want['k']]), c.name
    assert len(clusters) == want['k']
    for q, idx in enumerate(clusters):
        assert np.array_equal(idx.numpy(), want['order'][want['assign'][want['order']] == q]), (c.name, q)


@pytest.mark.parametrize('n', R.NMC_SIZES)
def test_nmc_box_counts(n):
    c = R.nmc_size_case(n)
    _check_nmc_direct(c)
    _check_nmc_wrapper(c)


@pytest.mark.parametrize('name', [c[0] for c in R.WINDOW_CASES])
def test_nmc_window_search(name):
    c = R.window_case(name)
    want = _check_nmc_direct(c)
    assert R.window_skips(want['found']) == c.skips
    _check_nmc_wrapper(c)


@pytest.mark.parametrize('name', R.NMC_EDGE_CASES)
def test_nmc_ties_iou_edges_degenerate_and_non_finite(name):
    """The two `zeros:` cases differed before the key of nmc_scene was built from score + 0.0f: a +0.0 box was visited before a
    -0.0 box of a lower row (profiles/nms_rule.md)."""
    c = R.nmc_edge_case(name)
    _check_nmc_direct(c)
    _check_nmc_wrapper(c)


@pytest.mark.parametrize('name', R.MAXK_CASES)
def test_nmc_max_k(name):
    """Heat rows at or beyond max_k keep their sentinel; max_k = 0 goes with heat = NULL."""
    _check_nmc_direct(R.maxk_case(name))


def test_nmc_at_the_documented_ceiling():
    _check_nmc_direct(R.ceiling_case())


@pytest.mark.parametrize('what', ['n', 'th0', 'th1'])
def test_nmc_refusals_write_nothing(what):
    from box2mask_amd import _lib
    n = R.NMC_MAX_N + 1 if what == 'n' else 40
    th = {'n': 0.5, 'th0': 0.0, 'th1': 1.0}[what]
    boxes = _dev(np.zeros((n, 7), F))
    o = _nmc_buffers(n, 1)
    with pytest.raises(_lib.B2MError):
        _call_nmc(boxes, n, th, 1, o)
    torch.cuda.synchronize()
    assert int(o['k'].item()) == R.SENT_I and (_np(o['reps']) == R.SENT_I).all() and (_np(o['assign']) == R.SENT_I).all()
    assert (_np(o['order']) == -1).all() and (_np(o['heat']).view(np.uint32) == R.SENT_F.view(np.uint32)).all()
    desc = _dev(R.nmc_batch_desc([n], [1])[0])
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_nmc_batch', boxes.data_ptr(), desc.data_ptr(), 1, n, th, o['reps'].data_ptr(), o['assign'].data_ptr(),
                  o['heat'].data_ptr(), o['k'].data_ptr(), o['order'].data_ptr())
    torch.cuda.synchronize()
    assert int(o['k'].item()) == R.SENT_I and (_np(o['assign']) == R.SENT_I).all()


def test_nmc_batch_through_the_wrapper():
    """Seven scenes, two of them empty, one with more clusters than the rows the wrapper reserves: every scene equals the rule and
    the single-scene call; the slices do not overlap."""
    from box2mask_amd import iou_nms
    c = R.nmc_batch_case()
    devs = [_dev(b) if len(b) else torch.zeros((0, 7), dtype=torch.float32, device='cuda') for b in c.scenes]
    res = iou_nms.nmc_device_batch(devs, float(c.th))
    assert len(res) == len(c.scenes)
    spans = []
    for s, (b, r) in enumerate(zip(c.scenes, res)):
        if len(b) == 0:
            assert r is None
            continue
        n = len(b)
        want = R.nmc(b, c.th, n)
        one = iou_nms.nmc_device(devs[s], float(c.th))
        for got in (r, one):
            assert got.k == want['k'] == c.ks[s] and got.n == n, s
            assert np.array_equal(_np(got.reps)[:got.k], want['reps']), s
            assert np.array_equal(_np(got.assign), want['assign']), s
            assert np.array_equal(_np(got.order)[:n] & 0xFFFFFFFF, want['order']), s
            assert R.same_floats(_np(got.heat), want['heat'][:want['k']]), s
        for t in (r.reps, r.assign, r.order, r.heat):
            spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_nmc_batch_direct_with_sentinels():
    """b2m_nmc_batch on a table of its own: reserved heat rows below, at and above the cluster count; the WHOLE heat, reps,
    assign and k buffers equal the rule's, so nothing is written outside a scene's slice or past its max_k."""
    from box2mask_amd import _lib
    c = R.nmc_batch_case()
    ns = [len(b) for b in c.scenes]
    mks = [0, 1, 2, 4, 0, 6, 256]
    assert any(0 < mk < k for mk, k in zip(mks, c.ks)) and any(mk == k for mk, k in zip(mks, c.ks) if k) and any(mk > k for mk, k in zip(mks, c.ks) if k)
    desc, nb, nh, no = R.nmc_batch_desc(ns, mks)
    boxes = _dev(np.concatenate(c.scenes, 0))
    reps, assign = _full(nb, R.SENT_I, torch.int32), _full(nb, R.SENT_I, torch.int32)
    heat = _dev(np.full(nh + 5, R.SENT_F, F))
    order = _full(no, -1, torch.int64)
    k = _full(len(ns), R.SENT_I, torch.int32)
    _lib.call('b2m_nmc_batch', boxes.data_ptr(), _dev(desc).data_ptr(), len(ns), max(ns), float(c.th), reps.data_ptr(),
              assign.data_ptr(), heat.data_ptr(), k.data_ptr(), order.data_ptr())
    w_reps, w_assign, w_heat = np.full(nb, R.SENT_I, np.int32), np.full(nb, R.SENT_I, np.int32), np.full(nh + 5, R.SENT_F, F)
    got_order = _np(order)
    for s, b in enumerate(c.scenes):
        bo, n, npad, mk, ho, oo = desc[s].tolist()
        if n == 0:
            assert (got_order[oo:oo + npad] == -1).all(), s
            continue
        want = R.nmc(b, c.th, mk)
        w_reps[bo:bo + want['k']] = want['reps']
        w_assign[bo:bo + n] = want['assign']
        w_heat[ho:ho + mk * n] = want['heat'].reshape(-1)
        assert np.array_equal(got_order[oo:oo + n] & 0xFFFFFFFF, want['order']), s
    assert _np(k).tolist() == c.ks
    assert np.array_equal(_np(reps), w_reps) and np.array_equal(_np(assign), w_assign)
    assert R.same_floats(_np(heat), w_heat)


# ----------------------------------------------------------------------------- projection
def _project_scene(c):
    d = dict(heat=_dev(c.heat), sel=_dev(c.sel), fg_slot=_dev(c.fg_slot), seg2vox=_dev(c.seg2vox),
             bits=_full((c.ksel + 1, c.words), SENT_W, torch.int64))
    sc = dict(n_fg=c.n_fg, ksel=c.ksel, n_vox=c.n_vox, words=c.words)
    want = np.full((c.ksel + 1, c.words), SENT_W, np.uint64)
    want[:c.ksel] = R.project(c.heat, c.sel, c.fg_slot, c.seg2vox, c.th)
    return sc, d, want


def _check_project_batch(cases):
    from box2mask_amd import _lib
    built = [_project_scene(c) for c in cases]
    scenes, devs = [b[0] for b in built], [b[1] for b in built]
    table = _table(scenes, devs)
    _lib.call('b2m_mask_project_batch', table.data_ptr(), len(scenes), sum(c.ksel for c in cases), max(c.words for c in cases),
              float(R.PROJ_TH))
    for c, (_, d, want) in zip(cases, built):
        assert np.array_equal(_np(d['bits']).view(np.uint64), want), c.name


@pytest.mark.parametrize('n_vox', R.PROJ_NVOX)
def test_mask_project_single_and_batch(n_vox):
    """Every ksel at this n_vox through b2m_mask_project, then all of them as one table through b2m_mask_project_batch."""
    from box2mask_amd import _lib
    cases = [R.project_case(n_vox, ksel) for ksel in R.PROJ_KSEL]
    for c in cases:
        _, d, want = _project_scene(c)
        _lib.call('b2m_mask_project', d['heat'].data_ptr(), c.n_fg, d['sel'].data_ptr(), c.ksel, d['fg_slot'].data_ptr(),
                  d['seg2vox'].data_ptr(), c.n_vox, float(c.th), d['bits'].data_ptr(), c.words)
        assert np.array_equal(_np(d['bits']).view(np.uint64), want), c.name
    _check_project_batch(cases)


def test_mask_project_batch_with_different_words_and_an_empty_scene():
    _check_project_batch([R.project_case(v, k) for v, k in R.PROJ_BATCH])


# ----------------------------------------------------------------------------- mask NMS
def _check_mask_nms_direct(c):
    from box2mask_amd import _lib
    k = c.k
    bits = _bits(c.bits)
    inter, keep, nk = _full(k * k + 1, R.SENT_I, torch.int32), _full(k + 1, R.SENT_I, torch.int32), _full(1, R.SENT_I, torch.int32)
    _lib.call('b2m_mask_nms', bits.data_ptr(), k, c.words, float(c.th), inter.data_ptr(), keep.data_ptr(), nk.data_ptr())
    w_inter, w_keep, w_nk = R.mask_nms(c.bits, c.th)
    got = _np(inter)
    assert np.array_equal(got[:k * k].reshape(k, k), w_inter) and got[-1] == R.SENT_I, c.name
    assert np.array_equal(_np(keep)[:k], w_keep) and _np(keep)[-1] == R.SENT_I, c.name
    assert int(nk.item()) == w_nk, c.name
    return w_keep


def _check_mask_nms_wrapper(c, w_keep):
    from box2mask_amd import iou_nms
    masks = R.unpack(c.bits, c.words * 64)
    kept, supp = iou_nms.mask_NMS(torch.from_numpy(masks), float(c.th), allow_empty=True)
    assert np.array_equal(kept.numpy(), np.flatnonzero(w_keep)), c.name
    assert [int(s[0]) for s in supp] == kept.tolist()
    gone = np.concatenate([s[1].numpy() for s in supp])            # (like the reference, each list starts with the kept row itself)
    assert np.array_equal(np.sort(gone), np.arange(c.k)), c.name


def _check_mask_nms_batch(scenes, th, max_k):
    from box2mask_amd import _lib
    devs = []
    for sc in scenes:
        k = sc['ksel']
        devs.append(dict(bits=_bits(sc['bits']), inter=_full(k * k + 1, R.SENT_I, torch.int32),
                         keep=_full(k + 1, R.SENT_I, torch.int32) if sc.get('has_keep', True) else None))
    table = _table(scenes, devs)
    _lib.call('b2m_mask_nms_batch', table.data_ptr(), len(scenes), max_k, float(th))
    for s, (sc, d) in enumerate(zip(scenes, devs)):
        k = sc['ksel']
        got = _np(d['inter'])
        if d['keep'] is None:
            assert (got == R.SENT_I).all(), s                       # no mask NMS for this scene: nothing written
            continue
        w_inter, w_keep, _ = R.mask_nms(sc['bits'], th)
        assert np.array_equal(got[:k * k].reshape(k, k), w_inter) and got[-1] == R.SENT_I, s
        assert np.array_equal(_np(d['keep'])[:k], w_keep) and _np(d['keep'])[-1] == R.SENT_I, s


@pytest.mark.parametrize('k', R.MNMS_K)
def test_mask_nms_row_and_word_counts(k):
    """k rows at every word count: b2m_mask_nms, mask_NMS (up to 257 rows) and the four scenes as one table through
    b2m_mask_nms_batch."""
    cases = [R.mask_nms_case(k, w) for w in R.MNMS_WORDS]
    for c in cases:
        w_keep = _check_mask_nms_direct(c)
        if k <= 257:
            _check_mask_nms_wrapper(c, w_keep)
    _check_mask_nms_batch([dict(ksel=k, words=c.words, n_vox=c.words * 64 - 5, bits=c.bits) for c in cases], cases[0].th, k)


@pytest.mark.parametrize('name', R.MNMS_EDGE_CASES)
def test_mask_nms_ratio_edges(name):
    c = R.mask_nms_edge_case(name)
    w_keep = _check_mask_nms_direct(c)
    if name != 'big_union':
        _check_mask_nms_wrapper(c, w_keep)
    _check_mask_nms_batch([dict(ksel=c.k, words=c.words, n_vox=c.words * 64, bits=c.bits)], c.th, c.k)


def test_mask_nms_batch_with_a_null_keep_scene_and_fewer_rows_than_max_k():
    c = R.mask_nms_batch_case()
    _check_mask_nms_batch(c.scenes, c.th, c.max_k)


# ----------------------------------------------------------------------------- label histogram
def _lh_devs(sc):
    return dict(bits=_bits(sc['bits']), rows=_dev(sc['rows']), sem=_dev(sc['sem']), labels=_full(sc['kk'] + 1, R.SENT_I, torch.int32))


def _lh_want(sc, n_class):
    want = np.full(sc['kk'] + 1, R.SENT_I, np.int32)
    if sc['kk']:
        want[:sc['kk']] = R.label_hist(sc['bits'], sc['rows'], sc['sem'], sc['n_vox'], n_class)
    return want


def _check_label_hist_batch(scenes, n_class):
    from box2mask_amd import _lib
    devs = [_lh_devs(sc) for sc in scenes]
    table = _table(scenes, devs)
    _lib.call('b2m_label_hist_batch', table.data_ptr(), len(scenes), sum(sc['kk'] for sc in scenes), n_class)
    for s, (sc, d) in enumerate(zip(scenes, devs)):
        assert np.array_equal(_np(d['labels']), _lh_want(sc, n_class)), (s, n_class)


@pytest.mark.parametrize('n_class', R.LH_NCLASS)
def test_label_hist_single_and_batch(n_class):
    from box2mask_amd import _lib
    cases = [R.label_hist_case(w, n_class, s) for w in R.LH_WORDS for s in (False, True)]
    scenes = []
    for c in cases:
        sc = dict(bits=c.bits, words=c.words, n_vox=c.n_vox, sem=c.sem, rows=c.rows, kk=c.kk, ksel=c.ksel)
        d = _lh_devs(sc)
        _lib.call('b2m_label_hist', d['bits'].data_ptr(), c.words, None if d['rows'] is None else d['rows'].data_ptr(), c.kk,
                  d['sem'].data_ptr(), c.n_vox, n_class, d['labels'].data_ptr())
        assert np.array_equal(_np(d['labels']), _lh_want(sc, n_class)), c.name
        scenes.append(sc)
    _check_label_hist_batch(scenes, n_class)
    _check_label_hist_batch(R.label_hist_batch_case(n_class).scenes, n_class)       # kk = 0 at the front, in the middle, at the end


def test_label_hist_refuses_more_than_256_classes():
    from box2mask_amd import _lib
    c = R.label_hist_case(1, 20, False)
    d = _lh_devs(dict(bits=c.bits, rows=None, sem=c.sem, kk=c.kk))
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_label_hist', d['bits'].data_ptr(), c.words, None, c.kk, d['sem'].data_ptr(), c.n_vox, 257, d['labels'].data_ptr())
    torch.cuda.synchronize()
    assert (_np(d['labels']) == R.SENT_I).all()


# ----------------------------------------------------------------------------- instance histogram
@pytest.mark.parametrize('words', R.MH_WORDS)
def test_mask_hist(words):
    from box2mask_amd import _lib
    for n_class in R.MH_NCLASS:
        for k in R.MH_K:
            c = R.mask_hist_case(words, n_class, k)
            bits, label = _bits(c.bits), _dev(c.label)
            hist = _full(k * n_class + 1, R.SENT_I, torch.int32)
            _lib.call('b2m_mask_hist', bits.data_ptr(), words, k, label.data_ptr(), c.n, n_class, hist.data_ptr())
            got = _np(hist)
            assert np.array_equal(got[:-1].reshape(k, n_class), R.mask_hist(c.bits, c.label, c.n, n_class)) and got[-1] == R.SENT_I, c.name
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_mask_hist', bits.data_ptr(), words, k, label.data_ptr(), c.n, R.HIST_MAX + 1, hist.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_np(hist), got)


# ----------------------------------------------------------------------------- gathers, pack, set_ious
@pytest.mark.parametrize('kk', R.GATHER_KK)
def test_mask_gathers(kk):
    """One table of ten scenes per kk: b2m_mask_gather_batch, b2m_mask_gather_batch_t and, scene by scene, b2m_mask_gather."""
    from box2mask_amd import _lib
    c = R.gather_batch_case(kk)
    scenes = c.scenes
    wants = []
    for sc in scenes:
        want = np.full(sc['kk'] * sc['n_pts'] + 64, R.SENT_B, np.uint8)
        want[:sc['kk'] * sc['n_pts']] = R.gather(sc['bits'], sc['rows'], sc['index'], sc['n_pts']).reshape(-1)
        wants.append(want)
    total, max_pts, max_words = sum(sc['kk'] for sc in scenes), max(sc['n_pts'] for sc in scenes), max(sc['words'] for sc in scenes)
    for entry in ('b2m_mask_gather_batch', 'b2m_mask_gather_batch_t', 'b2m_mask_gather'):
        devs = [dict(bits=_bits(sc['bits']), rows=_dev(sc['rows']), index=_dev(sc['index']),
                     out=_full(sc['kk'] * sc['n_pts'] + 64, R.SENT_B, torch.uint8)) for sc in scenes]
        if entry == 'b2m_mask_gather':
            for sc, d in zip(scenes, devs):
                _lib.call(entry, d['bits'].data_ptr(), sc['words'], _addr([d])(0, 'rows') or None, sc['kk'],
                          _addr([d])(0, 'index') or None, sc['n_pts'], d['out'].data_ptr())
        else:
            table = _table(scenes, devs)
            if entry.endswith('_t'):
                tb = [_full(max(sc['n_vox'] * ((sc['kk'] + 63) // 64), 1), 0, torch.int64) for sc in scenes]
                tptr = torch.tensor([t.data_ptr() for t in tb], dtype=torch.int64).cuda()
                _lib.call(entry, table.data_ptr(), len(scenes), total, max_pts, max_words, tptr.data_ptr())
            else:
                _lib.call(entry, table.data_ptr(), len(scenes), total, max_pts)
        torch.cuda.synchronize()
        for s, (d, want) in enumerate(zip(devs, wants)):
            assert np.array_equal(_np(d['out']), want), (entry, s, scenes[s]['n_pts'])


@pytest.mark.parametrize('n', R.PACK_N)
def test_mask_pack_takes_any_non_zero_byte(n):
    from box2mask_amd import _lib, iou_nms
    c = R.pack_case(n)
    k = len(c.masks)
    bits = _full((k + 1, c.words), SENT_W, torch.int64)
    _lib.call('b2m_mask_pack', _dev(c.masks).data_ptr(), k, n, bits.data_ptr(), c.words)
    want = np.full((k + 1, c.words), SENT_W, np.uint64)
    want[:k] = R.pack(c.masks)
    assert np.array_equal(_np(bits).view(np.uint64), want)
    b2, w2 = iou_nms.pack_masks(_dev(c.masks != 0))
    assert w2 == c.words and np.array_equal(_np(b2).view(np.uint64), want[:k])


@pytest.mark.parametrize('n', R.SET_N)
def test_set_ious(n):
    from box2mask_amd import _lib, iou_nms
    c = R.set_ious_case(n)
    out = _dev(np.full(n + 1, R.SENT_F, F))
    a, b = _dev(c.a), _dev(c.b)
    _lib.call('b2m_set_ious', a.data_ptr() if n else None, b.data_ptr() if n else None, n, out.data_ptr())
    want = np.concatenate([R.set_ious(c.a, c.b), [R.SENT_F]]).astype(F)
    assert R.same_floats(_np(out), want)
    assert R.same_floats(iou_nms.set_IOUs(torch.from_numpy(c.a), torch.from_numpy(c.b)).numpy(), want[:n])
