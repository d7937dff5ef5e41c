"""CPU: the host side of box2mask_amd/mask_stages.py -- the B2M_MASK_DESC table builder against the independent rule of
tests/_nms_rule.py (``mask_desc``), and the score filter.  No GPU and no library: the table is built on the CPU device from fake,
distinct addresses."""
import types

import numpy as np
import pytest
import torch

import _nms_rule as R
from box2mask_amd import mask_stages as M

CPU = torch.device('cpu')


def _fake(address):
    return types.SimpleNamespace(data_ptr=lambda: address)


def _address(s, name):
    """Distinct per scene and field, 4 KiB apart."""
    return 0x10000000 + (s * len(R.MASK_FIELDS) + R.MASK_FIELDS.index(name)) * 0x1000


# (ksel, kk, n_vox) per scene: S = 1, 2, 3; ksel = 0 first, in the middle and last; kk = 0 and kk = ksel; words = 0, 1 and 2
TABLES = {
    'one': [(3, 3, 64)],
    'one_empty': [(0, 0, 65)],
    'two_first_empty': [(0, 0, 64), (4, 2, 65)],
    'three_middle_empty': [(2, 0, 65), (0, 0, 0), (5, 5, 64)],
    'three_last_empty': [(1, 1, 0), (3, 2, 65), (0, 0, 64)],
}


@pytest.mark.parametrize('keep', [True, False])
@pytest.mark.parametrize('name', sorted(TABLES))
def test_mask_table_equals_the_rule(name, keep):
    shapes = TABLES[name]
    S = len(shapes)
    sc = [dict(n_fg=7 + s, n_vox=n_vox, words=(n_vox + 63) // 64, fg_slot=_fake(_address(s, 'fg_slot')), s2v=_fake(_address(s, 'seg2vox')),
               sem_vox=_fake(_address(s, 'sem'))) for s, (_, _, n_vox) in enumerate(shapes)]
    assert {d['words'] for d in sc} <= {0, 1, 2}
    heats = [_fake(_address(s, 'heat')) for s in range(S)]
    sels = [np.arange(k)[::-1].copy() for k, _, _ in shapes]
    tab = M.MaskTable(sc, heats, sels, CPU, keep=keep)
    assert tab.ksels == [k for k, _, _ in shapes] and tab.total == sum(tab.ksels)
    assert tab.sel_all.dtype == torch.int32 and tab.bits_all.dtype == torch.int64 and tab.inter_all.dtype == torch.int32
    if tab.total:
        assert np.array_equal(tab.sel_all.numpy(), np.concatenate(sels))
    rows_ptr, labels_ptr = 0x70000000, 0x78000000
    index = [None if s % 2 else _fake(_address(s, 'index')) for s in range(S)]
    tab.set_kept([kk for _, kk, _ in shapes], rows_ptr, labels_ptr,
                 [(index[s], 100 + s, _fake(_address(s, 'out'))) for s in range(S)])

    # what the rule is told: the sizes, and every address with the running byte offsets the stages rely on
    sel_o = np.cumsum([0] + [4 * k for k, _, _ in shapes])
    bits_o = np.cumsum([0] + [8 * k * max(d['words'], 1) for (k, _, _), d in zip(shapes, sc)])
    inter_o = np.cumsum([0] + [4 * k * k for k, _, _ in shapes])
    kept_o = np.cumsum([0] + [4 * kk for _, kk, _ in shapes])

    def address(s, field):
        if field == 'sel':
            return tab.sel_all.data_ptr() + int(sel_o[s])
        if field == 'bits':
            return tab.bits_all.data_ptr() + int(bits_o[s])
        if field == 'inter':
            return tab.inter_all.data_ptr() + int(inter_o[s])
        if field == 'keep':
            return tab.keep_all.data_ptr() + int(sel_o[s]) if keep and shapes[s][0] else 0
        if field == 'rows':
            return rows_ptr + int(kept_o[s])
        if field == 'labels':
            return labels_ptr + int(kept_o[s])
        if field == 'index':
            return 0 if index[s] is None else _address(s, 'index')
        return _address(s, field)
    scenes = [dict(n_fg=d['n_fg'], ksel=k, n_vox=d['n_vox'], words=d['words'], kk=kk, n_pts=100 + s)
              for s, ((k, kk, _), d) in enumerate(zip(shapes, sc))]
    want = R.mask_desc(scenes, address)
    assert tab.FIELDS == R.MASK_FIELDS
    for f, field in enumerate(R.MASK_FIELDS):
        assert np.array_equal(tab.desc[:, f], want[:, f]), field
    assert tab.desc[:, 18].tolist() == np.cumsum([0] + tab.ksels[:-1]).tolist()                   # running sums
    assert tab.desc[:, 19].tolist() == np.cumsum([0] + [kk for _, kk, _ in shapes][:-1]).tolist()
    assert tab.row0 == tab.desc[:, 18].tolist() and tab.bits_ptr == tab.desc[:, 7].tolist()
    assert (tab.desc[:, 10] == 0).all() if not keep else all((p == 0) == (k == 0) for p, (k, _, _) in zip(tab.desc[:, 10], shapes))
    assert tab.sel_all.numel() >= max(tab.total, 1) and tab.inter_all.numel() >= int(inter_o[-1]) // 4
    assert tab.bits_all.numel() >= int(bits_o[-1]) // 8

    # the upload: the table, and the optional tail 8 * S * 20 bytes behind it
    tail = np.arange(3 * S, dtype=np.int64) + 5
    desc_ptr, extra_ptr = tab.upload(tail)
    assert desc_ptr == tab.table_dev.data_ptr() and extra_ptr - desc_ptr == 8 * S * 20
    assert np.array_equal(tab.table_dev.numpy(), np.concatenate([want.reshape(-1), tail]))
    desc_ptr, extra_ptr = tab.upload()
    assert extra_ptr - desc_ptr == 8 * S * 20 and np.array_equal(tab.table_dev.numpy(), want.reshape(-1))


def test_mask_table_without_rows_and_gather():
    """The sweeps' use: every projected row is kept (rows = NULL), nothing is gathered."""
    sc = [dict(n_fg=3, n_vox=65, words=2, fg_slot=_fake(8), s2v=_fake(16), sem_vox=_fake(24 + 8 * s)) for s in range(2)]
    tab = M.MaskTable(sc, [_fake(64), _fake(128)], [np.arange(2), np.arange(3)], CPU)
    tab.set_kept(tab.ksels, 0, 0x5000)
    f = R.MASK_FIELDS.index
    assert tab.desc[:, f('rows')].tolist() == [0, 0] and tab.desc[:, f('kk')].tolist() == [2, 3]
    assert tab.desc[:, f('labels')].tolist() == [0x5000, 0x5008] and tab.desc[:, f('sem')].tolist() == [24, 32]
    assert tab.desc[:, f('row0_kept')].tolist() == [0, 2] and not tab.desc[:, f('index'):f('out') + 1].any()
    assert not tab.desc[:, f('keep')].any()


def test_score_filter_is_strict_after_float32():
    conf = np.array([0.9, 0.3, 0.3, 0.1], np.float32)
    ths = [0.1, 0.3, 0.30000001192092896, 0.95]
    assert M.score_prefixes(conf, ths).tolist() == [3, 1, 1, 0]
    assert M.score_prefixes(conf, ths).dtype == np.int64
    for th, k in zip(ths, [3, 1, 1, 0]):
        got = M.score_filter(conf, th)
        assert got.dtype == np.int64 and got.tolist() == list(range(k))


def test_a_nan_score_is_no_prefix():
    conf = np.array([0.9, np.nan, 0.5, 0.1], np.float32)
    with pytest.raises(ValueError, match='did not keep a prefix'):
        M.score_prefixes(conf, [0.2])
    assert M.score_filter(conf, 0.2).tolist() == [0, 2]               # the single-setting filter: the rows as they are
    assert M.score_prefixes(conf, [0.95]).tolist() == [0]             # nothing kept is a prefix
