"""GPU: the packed weight images, byte for byte against a numpy restatement of their documented layout (include/b2m.h:
b2m_weight_pack, b2m_conv_fwd_h; csrc/conv.hip above pack_pos and conv_h_ck).  Every image is packed twice -- through the one-image
entry (b2m_weight_pack, b2m_weight_pack_h, b2m_weight_pack_h_t) and as the second image of a two-image plan, behind a one-block
image, so that the fp32 kernel crosses a descriptor boundary inside a workgroup -- into buffers pre-filled with a sentinel and one
element longer than b2m_weight_pack_size / _h_size: the padding is exactly zero, the extra element untouched.  The shapes are the
smallest that reach every path of the packers: the generic block (8-channel chunks), the <16,3> and <16,2> blocks, several chunks
and strips, partial chunks and strips, a row pitch that is no multiple of 4 (scalar loads), transposed images with and without
the mirror at slices whose start is and is not a multiple of 4; half images of 32- and 16-channel chunks, 2, 3 and 4 tiles per
strip, two sources, a pitched source, transposed slices.  (By conv_h_ck a 32-channel layer is ONE 32-channel chunk and is packed
in 16s: the half cases 27 | 64 x 64 and the transposed 8 | cout 64 are the ones that reach 32-channel chunks -- keep them.)"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENT32, SENT16 = 0x5A5A5A5A, 0x5A5A


# ----------------------------------------------------------------------------- the layouts, restated
def _logical(w, transpose, mirror, s0, sc):
    """B[k][ci][co], the operand an image holds, of weights w (K, cin, cout)."""
    if not transpose:
        return w
    src = w[::-1] if mirror else w
    return np.ascontiguousarray(src[:, s0:s0 + sc, :].transpose(0, 2, 1))


def _gather(B, k, ci, co):
    K, CI, CO = B.shape
    ok = (ci < CI) & (co < CO)
    return np.where(ok, B[k, np.minimum(ci, CI - 1), np.minimum(co, CO - 1)], B.dtype.type(0))


def image_f32(B):
    K, CI, CO = B.shape
    KC = 16 if CI >= 16 else 8
    TW = 3 if (CO % 48 == 0 and K > 1) else 2
    KS, SW, FPL = KC // 4, 16 * TW, TW * (KC // 4)
    LW = 64 * FPL
    nchunk, nstrip = -(-CI // KC), -(-CO // SW)
    e = np.arange(K * nstrip * nchunk * LW, dtype=np.int64)
    blk, pos = e // LW, e % LW
    if FPL % 4 == 0:                                     # [f / 4][lane][f % 4]
        lane, f = (pos & 255) >> 2, (pos >> 8) * 4 + (pos & 3)
    else:                                                # [lane][f]
        lane, f = pos // FPL, pos % FPL
    chunk, strip, k = blk % nchunk, (blk // nchunk) % nstrip, blk // (nchunk * nstrip)
    s, t, q, i = f // TW, f % TW, lane >> 4, lane & 15
    return _gather(B, k, chunk * KC + KS * q + s, strip * SW + 16 * t + i)


def half_ck(c1, c2):
    if c1 % 32 == 0 and c2 % 32 == 0 and ((c1 + c2) // 32 % 2 == 0 or (c1 + c2) // 32 % 3 == 0):
        return 32
    return 16


def image_f16(B, c1, c2):
    K, CI, CO = B.shape
    CK = half_ck(c1, c2)
    TW = 4 if (K > 1 and CO % 64 == 0) else 3 if (CO % 48 == 0 and K > 1) else 2
    E, SW = CK // 4, 16 * TW
    BLK = 64 * TW * E
    nchunk, nstrip = CI // CK, -(-CO // SW)
    e = np.arange(K * nstrip * nchunk * BLK, dtype=np.int64)
    blk, pos = e // BLK, e % BLK
    t, lane, j = pos // (64 * E), (pos // E) % 64, pos % E
    chunk, strip, k = blk % nchunk, (blk // nchunk) % nstrip, blk // (nchunk * nstrip)
    return _gather(B, k, chunk * CK + E * (lane >> 4) + j, strip * SW + 16 * t + (lane & 15)).astype(np.float16)


# ----------------------------------------------------------------------------- the cases
def _weights(K, cin, cout, seed):
    return np.random.default_rng(seed).standard_normal((K, cin, cout)).astype(np.float32)


# (K, cin, cout, transpose, mirror, slice begin, slice count, extra row pitch)
F32_CASES = [(1, 8, 32, 0, 0, 0, 0, 0), (27, 16, 48, 0, 0, 0, 0, 0), (27, 16, 32, 0, 0, 0, 0, 0), (27, 32, 64, 0, 0, 0, 0, 0),
             (1, 96, 3, 0, 0, 0, 0, 0), (8, 20, 36, 0, 0, 0, 0, 0), (27, 16, 32, 0, 0, 0, 0, 8)]
F32_CASES += [(27, 32, 48, 1, m, s0, sc, 0) for m in (0, 1) for s0, sc in ((0, 16), (16, 16), (2, 20))]
# (K, cin, cout, c1, transposed, mirror, slice begin, slice count, extra row pitch (one-image entry only))
F16_CASES = [(27, 32, 64, 32, 0, 0, 0, 0, 0), (27, 64, 64, 64, 0, 0, 0, 0, 0), (27, 48, 48, 48, 0, 0, 0, 0, 0),
             (1, 32, 32, 16, 0, 0, 0, 0, 0), (27, 48, 48, 48, 0, 0, 0, 0, 8),
             (27, 96, 32, 0, 1, 0, 32, 64, 0), (27, 96, 32, 0, 1, 1, 32, 64, 0), (8, 32, 64, 0, 1, 1, 0, 32, 0)]


def _sentinel(n, half):
    return torch.full((n + 1,), SENT16 if half else SENT32, dtype=torch.int16 if half else torch.int32, device='cuda')


def _same(buf, want, tag):
    got = buf.cpu().numpy()
    bits = np.uint16 if want.dtype == np.float16 else np.uint32
    assert len(got) == len(want) + 1, (tag, len(got), len(want))
    assert np.array_equal(got[:-1].view(bits), want.view(bits)), (tag, 'image')
    assert got[-1:].view(bits)[0] == (SENT16 if bits is np.uint16 else SENT32), (tag, 'written past the image')


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _device_weights(w, pad):
    """w with `pad` more floats per row (NaN: a read past the columns shows)"""
    K, cin, cout = w.shape
    wd = torch.full((K, cin, cout + pad), float('nan'), device='cuda')
    wd[:, :, :cout] = torch.from_numpy(w).cuda()
    return wd


def _blocks_f32(K, CI, CO):
    KC = 16 if CI >= 16 else 8
    SW = 16 * (3 if (CO % 48 == 0 and K > 1) else 2)
    return K * -(-CO // SW) * -(-CI // KC)


@pytest.mark.parametrize('case', F32_CASES, ids=lambda c: 'K%d_%dx%d_t%d_m%d_s%d_%d_p%d' % c)
def test_fp32_image_is_the_documented_layout_through_the_entry_and_through_a_plan(case):
    from box2mask_amd import _lib
    lib = _lib.load()
    K, cin, cout, tr, mirror, s0, sc, pad = case
    w = _weights(K, cin, cout, 7)
    want = image_f32(_logical(w, tr, mirror, s0, sc))
    CI, CO = (cout, sc) if tr else (cin, cout)
    assert lib.b2m_weight_pack_size(K, CI, CO) == len(want)
    ldw, wd = cout + pad, _device_weights(w, pad)
    one = _sentinel(len(want), False)
    _lib.call('b2m_weight_pack', wd.data_ptr(), ldw, K, cin, cout, tr, mirror, s0, sc, one.data_ptr())
    _same(one, want, 'entry')
    # a plan of two: a one-block image first, so that this image starts inside a workgroup's run of blocks
    lead = _weights(1, 8, 32, 3)
    lead_want = image_f32(lead)
    ld, b0, b1 = torch.from_numpy(lead).cuda(), _sentinel(len(lead_want), False), _sentinel(len(want), False)
    cols = [_i64([ld.data_ptr(), wd.data_ptr()]), _i64([b0.data_ptr(), b1.data_ptr()]), _i64([32, ldw]), _i32([1, K]), _i32([8, cin]),
            _i32([32, cout]), _i32([0, tr]), _i32([0, mirror]), _i32([0, s0]), _i32([0, sc])]
    host = np.zeros(2 * lib.b2m_weight_pack_plan_size(), np.uint8)
    blocks = lib.b2m_weight_pack_plan(2, *[_p(c) for c in cols], _p(host))
    assert blocks == 1 + _blocks_f32(K, CI, CO), lib.b2m_last_error().decode()       # a workgroup per 8 of them
    plan = torch.from_numpy(host).cuda()
    _lib.call('b2m_weight_pack_run', plan.data_ptr(), 2, blocks)
    _same(b0, lead_want, 'plan, first image')
    _same(b1, want, 'plan')


@pytest.mark.parametrize('case', F16_CASES, ids=lambda c: 'K%d_%dx%d_c%d_t%d_m%d_s%d_%d_p%d' % c)
def test_half_image_is_the_documented_layout_through_the_entry_and_through_a_plan(case):
    from box2mask_amd import _lib
    lib = _lib.load()
    K, cin, cout, c1, tr, mirror, s0, sc, pad = case
    w = _weights(K, cin, cout, 11)
    a1, a2, CO = (cout, 0, sc) if tr else (c1, cin - c1, cout)
    want = image_f16(_logical(w, tr, mirror, s0, sc), a1, a2)
    assert lib.b2m_weight_pack_h_size(K, a1, a2, CO) == len(want)
    ldw, wd = cout + pad, _device_weights(w, pad)
    one = _sentinel(len(want), True)
    if tr:
        _lib.call('b2m_weight_pack_h_t', wd.data_ptr(), K, cin, cout, mirror, s0, sc, one.data_ptr())
    else:
        _lib.call('b2m_weight_pack_h', wd.data_ptr(), ldw, K, c1, cin - c1, cout, one.data_ptr())
    _same(one, want, 'entry')
    if pad:
        return                                           # (a plan's weights are contiguous)
    lead = _weights(1, 16, 32, 5)
    lead_want = image_f16(lead, 16, 0)
    ld, b0, b1 = torch.from_numpy(lead).cuda(), _sentinel(len(lead_want), True), _sentinel(len(want), True)
    cols = [_i64([ld.data_ptr(), wd.data_ptr()]), _i64([b0.data_ptr(), b1.data_ptr()]), _i32([1, K]), _i32([16, cin]), _i32([32, cout]),
            _i32([16, c1]), _i32([0, tr]), _i32([0, mirror]), _i32([0, s0]), _i32([0, sc])]
    host = np.zeros(2 * lib.b2m_weight_pack_h_plan_size(), np.uint8)
    blocks = lib.b2m_weight_pack_h_plan(2, *[_p(c) for c in cols], _p(host))
    assert blocks == 1 + -(-len(want) // 2048), lib.b2m_last_error().decode()
    plan = torch.from_numpy(host).cuda()
    _lib.call('b2m_weight_pack_h_run', plan.data_ptr(), 2, blocks)
    _same(b0, lead_want, 'plan, first image')
    _same(b1, want, 'plan')


def test_the_packers_refuse_a_bad_slice_and_channels_that_do_not_come_in_16s():
    from box2mask_amd import _lib
    lib = _lib.load()
    w = torch.zeros(27 * 32 * 48, device='cuda')
    out = _sentinel(27 * 48 * 48, False)
    for s0, sc in ((-1, 16), (24, 16), (0, 0)):
        with pytest.raises(_lib.B2MError, match='b2m_weight_pack: bad channel slice'):
            _lib.call('b2m_weight_pack', w.data_ptr(), 48, 27, 32, 48, 1, 0, s0, sc, out.data_ptr())
    with pytest.raises(_lib.B2MError, match='b2m_weight_pack: bad arguments'):
        _lib.call('b2m_weight_pack', w.data_ptr(), 40, 27, 32, 48, 0, 0, 0, 0, out.data_ptr())       # pitch below cout
    with pytest.raises(_lib.B2MError, match='multiples of 16'):
        _lib.call('b2m_weight_pack_h', w.data_ptr(), 48, 27, 24, 8, 48, out.data_ptr())
    with pytest.raises(_lib.B2MError, match='multiple of 16'):
        _lib.call('b2m_weight_pack_h_t', w.data_ptr(), 27, 48, 24, 0, 0, 16, out.data_ptr())
    with pytest.raises(_lib.B2MError, match='b2m_weight_pack_h_t: bad arguments'):
        _lib.call('b2m_weight_pack_h_t', w.data_ptr(), 27, 32, 48, 0, 24, 16, out.data_ptr())
    assert (out.cpu().numpy().view(np.uint32) == SENT32).all()                  # refused on the host: nothing launched
    host = np.zeros(lib.b2m_weight_pack_plan_size(), np.uint8)
    cols = [_i64([w.data_ptr()]), _i64([out.data_ptr()]), _i64([48]), _i32([27]), _i32([32]), _i32([48]), _i32([1]), _i32([0]), _i32([24]), _i32([16])]
    assert lib.b2m_weight_pack_plan(1, *[_p(c) for c in cols], _p(host)) < 0
    assert 'b2m_weight_pack_plan: bad channel slice' in lib.b2m_last_error().decode()
