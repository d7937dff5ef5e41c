"""The convolution kernels (csrc/conv.hip, conv_fwd_flow.h, conv_1x1.h) against the float64 rule of tests/_conv_rule.py at the
edges where they can go wrong, through the product's entry points -- bit for bit on operands for which fp32 arithmetic is exact in
any order (torch.equal, no tolerance), and inside a derived bound on full-mantissa operands with short sums.

Neighbour tables are handed to sparse.Rulebook directly (the map-building code has bit-exact tests of its own); the transposed and
strided maps come from CoordinateManager on hand-placed coordinates with the rule's tables from oracle.sparse_ref.

THE MATRIX (every listed value of every axis appears at least once; not the cross product)

  LAYERS: forward (conv_raw), data gradient per source (conv_raw over the reverse table with the transposed image), weight gradient
  onto a non-zero dW0 (wgrad_raw, the second source at ci0 > 0).  mode: plain | bias | acc (accumulate onto y0) | bias_acc | wide
  (into columns of a wider 16-byte-aligned buffer whose other columns must stay as they were).  view: how x reaches the kernel.

    id   table      K   n_out<-n_in   cin       cout  mode      view                        what it reaches
    L0   dense      27  1<-1          16        16    plain     -                           one row, one chunk, zero slab
    L1   mixed      27  63<-63        32        32    bias      -                           partial single tile
    L2   dense      8   64<-100       48        48    acc       -                           K = 8, odd chunk count, 48-column strip, n_in > n_out
    L3   random     27  65<-65        64        80    bias_acc  -                           two tiles, half-filled last strip
    L4   mixed      8   129<-64       96        96    wide      -                           n_in < n_out, library zero-fill of a pitched output
    L5   dense      27  129<-129      256|128   256   plain     -                           two sources, every visit full, 24 chunks
    L6   random     27  511<-511      256       16    bias      -                           last size under the 8-tile cap / zero slab
    L7   mixed      27  512<-512      96        3     acc       -                           8 tiles; cout 3: vec_store = 0 with K > 1
    L8   mixed      27  513<-513      20        13    bias_acc  -                           per-element variant (cin 20), cout 13
    L9   broadcast  27  513<-300      32        96    plain     -                           one input row for all outputs, row n_in - 1
    L10  random     8   700<-900      96        32    wide      odd pitch (97)              per-element variant by pitch, level-5 size
    L11  mixed      27  4032<-4032    64        48    bias      column slice, pitch 80      63 tiles, empty tiles
    L12  mixed      27  4033<-4033    96|32     96    acc       -                           64 tiles: balanced XCD order, zero-cost tiles
    L13  last_row   27  4033<-4033    16        32    bias_acc  -                           a single pair in the last row of the last tile
    L14  centre     27  700<-700      48        256   plain     -                           one offset, widest output

  Every layer runs under the default dispatch; each switch on the layers whose launches it can change:

    B2M_CONV_TARGET=0        L1 L3 L5 L8 L12      B2M_CONV_MAXSLICE=16     L3 L5 L7 L12
    B2M_CONV_WGCOMBINE=0     L2 L5 L6 L12         B2M_CONV_CHUNKSPLIT=0    L5 L6 L12
    B2M_CONV_HANDLOADS=0     L1 L5 L11 L12        B2M_DETERMINISTIC=1      L0 L4 L5 L7 L12 (weight gradient twice: same bits)
    B2M_CONV_FAST32=0        L3 L5 L10 L12        B2M_WGRAD_PIPE=0         L2 L5 L12     B2M_WGRAD_KPACK=0   L1 L13
    B2M_WGRAD_MIN_TILES=64   L5 L11 L12           B2M_WGRAD_FAST32=0       L3 L12

  STEM  K = 125: 6 -> 32 through sparse_conv (pads the input), 8 -> 32 through conv_raw; rows 65 and 4033; B2M_CONV_STEM 1 | 0,
        un-split (B2M_CONV_TARGET=0, the form the stem kernel takes) and the default (split) dispatch.
  1x1   cin 16 | 96 | 96+32 | 320, cout 1 | 3 | 13 | 20 | 32 | 96 | 128 (1, 2, 3 strips per wave: the last two need 1024 / 2048 tiles),
        n_in = n_out and n_in > n_out, bias / accumulate, B2M_CONV_1X1=0.
  EPILOGUE  conv_affine with / without residual and ReLU on shapes it fuses and shapes it must refuse: cout % 4 != 0, which is also
        the only way a residual pitch reaches the library misaligned (conv_affine makes the residual's rows contiguous); behind the
        refusal b2m_bn_apply runs one element per thread (test_per_element_apply_equals_the_vector_kernel).
  TILE STATISTICS  un-split, 4-slice, two-slice: both sums exact (partial last tile; accumulate un-split); > 4 slices: list empty.
  MAPS  CoordinateManager: one coarse cell with 1 | 2 | 8 children, 65 coarse cells, a random 30 % grid (~3 k fine rows); strided
        and transposed layers through sparse_conv + backward; B2M_CONV_UP_MIN_ITEMS=1 | B2M_CONV_UP=0 | B2M_WGRAD_UP=0.
  WEIGHT GRADIENT  block shapes of pick_blk 1..4 (16->16 single accumulator: the plain kernel; 32->32, 8->32, 32->96 K-packed;
        48->48, 64->64, 96->96, 128->128), an overhanging block (cin 80, pitch 80 and pitch 128), narrow 1x1 outputs (3, 13).
  HALF  half_train.conv + backward, conv_affine_h / weight_pack_h: rows 1 | 65 | 513 | 4033, channels 32 | 96 | 96+32 | 256, one case
        per table kind and map kind, the three weight-gradient forms; one short-sum full-mantissa case per kernel.
  ARITHMETIC  full-mantissa operands, T <= 64, rows 65 and 4033, cin 16 | 32: general, flow, stem, 1x1, scatter-form up, plain and
        pipelined weight gradient, narrow weight gradient.  Observed error / bound ratios: profiles/conv_rule.md.
  EMPTY  n_out = 0 and n_in = 0 through every entry above.
"""
import ctypes

import numpy as np
import pytest
import torch

import _conv_rule as R

pytestmark = pytest.mark.gpu

# id: (table, K, n_out, n_in, c1, c2, cout, mode, view)
LAYERS = {
    'L0': ('dense', 27, 1, 1, 16, 0, 16, 'plain', None),
    'L1': ('mixed', 27, 63, 63, 32, 0, 32, 'bias', None),
    'L2': ('dense', 8, 64, 100, 48, 0, 48, 'acc', None),
    'L3': ('random', 27, 65, 65, 64, 0, 80, 'bias_acc', None),
    'L4': ('mixed', 8, 129, 64, 96, 0, 96, 'wide', None),
    'L5': ('dense', 27, 129, 129, 256, 128, 256, 'plain', None),
    'L6': ('random', 27, 511, 511, 256, 0, 16, 'bias', None),
    'L7': ('mixed', 27, 512, 512, 96, 0, 3, 'acc', None),
    'L8': ('mixed', 27, 513, 513, 20, 0, 13, 'bias_acc', None),
    'L9': ('broadcast', 27, 513, 300, 32, 0, 96, 'plain', None),
    'L10': ('random', 8, 700, 900, 96, 0, 32, 'wide', 'odd_pitch'),
    'L11': ('mixed', 27, 4032, 4032, 64, 0, 48, 'bias', 'slice'),
    'L12': ('mixed', 27, 4033, 4033, 96, 32, 96, 'acc', None),
    'L13': ('last_row', 27, 4033, 4033, 16, 0, 32, 'bias_acc', None),
    'L14': ('centre', 27, 700, 700, 48, 0, 256, 'plain', None),
}
SWITCHES = {
    'default': ({}, sorted(LAYERS, key=lambda s: int(s[1:]))),
    'unsplit': ({'B2M_CONV_TARGET': '0'}, ['L1', 'L3', 'L5', 'L8', 'L12']),
    'maxslice16': ({'B2M_CONV_MAXSLICE': '16'}, ['L3', 'L5', 'L7', 'L12']),
    'atomic_combine': ({'B2M_CONV_WGCOMBINE': '0'}, ['L2', 'L5', 'L6', 'L12']),
    'no_chunk_slices': ({'B2M_CONV_CHUNKSPLIT': '0'}, ['L5', 'L6', 'L12']),
    'compiler_tracked_loads': ({'B2M_CONV_HANDLOADS': '0'}, ['L1', 'L5', 'L11', 'L12']),
    'deterministic': ({'B2M_DETERMINISTIC': '1'}, ['L0', 'L4', 'L5', 'L7', 'L12']),
    'fwd_64bit': ({'B2M_CONV_FAST32': '0'}, ['L3', 'L5', 'L10', 'L12']),
    'wgrad_plain': ({'B2M_WGRAD_PIPE': '0'}, ['L2', 'L5', 'L12']),
    'wgrad_no_kpack': ({'B2M_WGRAD_KPACK': '0'}, ['L1', 'L13']),
    'wgrad_64_tile_chunks': ({'B2M_WGRAD_MIN_TILES': '64'}, ['L5', 'L11', 'L12']),
    'wgrad_64bit': ({'B2M_WGRAD_FAST32': '0'}, ['L3', 'L12']),
}


def _dev(t):
    return None if t is None else t.cuda()


def _rulebook(nbr, n_in):
    from box2mask_amd.sparse import Rulebook
    K, n_out = nbr.shape
    return Rulebook(torch.from_numpy(np.ascontiguousarray(nbr)).cuda(), K, n_out, n_in)


def _view(t, how):
    """The device tensor the kernel reads: contiguous, a view with an odd row pitch, or a column slice of a wider tensor."""
    t = t.cuda()
    if how is None:
        return t
    n, c = t.shape
    if how == 'odd_pitch':
        wide = torch.full((n, c + 1), 9.0, device='cuda')
        wide[:, :c] = t
        return wide[:, :c]
    if how == 'slice':                                   # columns 8 .. 8 + c of a pitch-(c + 16) tensor: 16-byte aligned rows
        wide = torch.full((n, c + 16), 9.0, device='cuda')
        wide[:, 8:8 + c] = t
        return wide[:, 8:8 + c]
    if how.startswith('pitch'):                          # zero-padded rows of a wider pitch (what the stem's 6-channel input gets)
        wide = torch.zeros((n, int(how[5:])), device='cuda')
        wide[:, :c] = t
        return wide[:, :c]
    raise ValueError(how)


_refs = {}


def _layer_ref(name):
    """Tables, operands and every float64 reference of a layer, with the exactness condition asserted -- once per module."""
    if name in _refs:
        return _refs[name]
    table, K, n_out, n_in, c1, c2, cout, mode, view = LAYERS[name]
    nbr = R.table(table, K, n_out, n_in, seed=11)
    ops = R.exact_operands(11, n_in, c1, c2, K, cout, n_out)
    g = ops['g']
    bias = ops['bias'] if 'bias' in mode else None
    y0 = ops['y0'] if 'acc' in mode else None
    ref = {'nbr': nbr, 'ops': ops, 'bias': bias, 'y0': y0}
    ref['fwd'] = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], bias, y0)
    R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w'], bias, y0), ref['fwd'], g)
    if R.has_reverse(nbr):
        ref['rev'] = R.reverse_table(nbr, n_in)
        for s, (c0, c) in enumerate(((0, c1), (c1, c2))):
            if c:
                dx0 = ops['dx0'][:, c0:c0 + c].contiguous() if s == 1 or 'acc' in mode else None
                ref['dx%d' % s] = (R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in, c0, c, dx0), dx0)
                R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n_in, c0, c, dx0), ref['dx%d' % s][0], g)
    dw = ops['dw0'].double()
    for x, ci0 in ((ops['x1'], 0), (ops['x2'], c1)):
        if x is not None:
            R.assert_exact(R.S_wgrad(nbr, x, ops['dy'], dw, ci0), R.conv_wgrad(nbr, x, ops['dy'], dw, ci0), 1.0)
            dw = R.conv_wgrad(nbr, x, ops['dy'], dw, ci0)
    ref['dw'] = dw
    _refs[name] = ref
    return ref


def _forward(ops, rb, K, n_out, cout, bias, y0, mode, view, x1=None, x2=None):
    from box2mask_amd import functional as F_
    x1 = _view(ops['x1'], view) if x1 is None else x1
    x2 = _dev(ops['x2']) if x2 is None else x2
    wp = F_.weight_pack(ops['w'].cuda())
    out, marker = None, None
    if mode == 'wide':
        marker = torch.full((n_out, cout + 12), -7.0, device='cuda')
        out = marker[:, 4:4 + cout]
    elif y0 is not None:
        out = y0.cuda().clone()
    y = F_.conv_raw(x1, x2, wp, K, _dev(bias), rb, n_out, cout, out=out, accumulate=y0 is not None)
    torch.cuda.synchronize()
    if marker is not None:
        assert y.data_ptr() == out.data_ptr()
        keep = torch.ones(cout + 12, dtype=torch.bool); keep[4:4 + cout] = False
        assert bool((marker.cpu()[:, keep] == -7.0).all()), 'columns outside the output were written'
    return y


@pytest.mark.parametrize('switch,name', [pytest.param(s, n, id='%s-%s' % (s, n)) for s in SWITCHES for n in SWITCHES[s][1]])
def test_layer_is_the_rule_bit_for_bit(monkeypatch, switch, name):
    from box2mask_amd import functional as F_
    table, K, n_out, n_in, c1, c2, cout, mode, view = LAYERS[name]
    ref = _layer_ref(name)
    ops, nbr = ref['ops'], ref['nbr']
    for k, v in SWITCHES[switch][0].items():
        monkeypatch.setenv(k, v)
    rb = _rulebook(nbr, n_in)
    y = _forward(ops, rb, K, n_out, cout, ref['bias'], ref['y0'], mode, view)
    assert R.same(y, ref['fwd']), 'forward: %d elements differ, max %.4g' % (
        int((y.cpu().double() != ref['fwd']).sum()), float((y.cpu().double() - ref['fwd']).abs().max()))
    # data gradient: the forward kernel over the reverse table with the transposed image of each source's slice
    if 'rev' in ref:
        rbr = _rulebook(ref['rev'], n_out)
        dy = _dev(ops['dy'])
        for s, (c0, c) in enumerate(((0, c1), (c1, c2))):
            if not c:
                continue
            want, dx0 = ref['dx%d' % s]
            wt = F_.weight_pack(ops['w'].cuda(), True, False, c0, c)
            acc = dx0.cuda().clone() if dx0 is not None else None
            dx = F_.conv_raw(dy, None, wt, K, None, rbr, n_in, c, out=acc, accumulate=acc is not None)
            assert R.same(dx, want), 'data gradient of source %d: max %.4g' % (s, float((dx.cpu().double() - want).abs().max()))
    # weight gradient onto dW0, the second source at ci0 = c1
    runs = []
    for _ in range(2 if switch == 'deterministic' else 1):
        dw = ops['dw0'].cuda().clone()
        F_.wgrad_raw(_view(ops['x1'], None if view == 'odd_pitch' else view), _dev(ops['dy']), rb, K, dw, 0, c1)
        if c2:
            F_.wgrad_raw(_dev(ops['x2']), _dev(ops['dy']), rb, K, dw, c1, c2)
        runs.append(dw.cpu())
        assert R.same(dw, ref['dw']), 'weight gradient: max %.4g' % float((dw.cpu().double() - ref['dw']).abs().max())
    assert all(torch.equal(r, runs[0]) for r in runs)


# ------------------------------------------------------------------ stem
@pytest.mark.parametrize('env', [{'B2M_CONV_STEM': '1', 'B2M_CONV_TARGET': '0'}, {'B2M_CONV_STEM': '0', 'B2M_CONV_TARGET': '0'},
                                 {'B2M_CONV_STEM': '1'}, {'B2M_CONV_STEM': '0'}], ids=lambda e: '-'.join('%s=%s' % kv for kv in e.items()))
@pytest.mark.parametrize('n', [65, 4033])
def test_stem_layer_is_the_rule_bit_for_bit(monkeypatch, n, env):
    """K = 125: 6 -> 32 through the autograd operator (which pads the 6-channel rows) with its backward pass, 8 -> 32 through
    conv_raw with bias and accumulate."""
    from box2mask_amd import functional as F_
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('B2M_WGRAD_STREAM', '0')
    K = 125
    nbr = R.table('mixed', K, n, n, seed=5)
    rb = _rulebook(nbr, n)
    rbr = _rulebook(R.reverse_table(nbr, n), n)
    ops = R.exact_operands(5, n, 6, 0, K, 32, n)
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'])
    R.assert_exact(R.S_fwd(nbr, ops['x1'], None, ops['w'], ops['bias']), ref, ops['g'])
    x = ops['x1'].cuda().requires_grad_(True); w = ops['w'].cuda().requires_grad_(True); b = ops['bias'].cuda().requires_grad_(True)
    y = F_.sparse_conv(x, None, w, b, rb, rbr, False, n)
    y.backward(ops['dy'].cuda())
    torch.cuda.synchronize()
    assert R.same(y, ref)
    want = R.conv_dgrad(nbr, ops['dy'], ops['w'], n)
    R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n), want, ops['g'])
    assert R.same(x.grad, want)
    want = R.conv_wgrad(nbr, ops['x1'], ops['dy'], torch.zeros(K, 6, 32))
    R.assert_exact(R.S_wgrad(nbr, ops['x1'], ops['dy'], torch.zeros(K, 6, 32)), want, 1.0)
    assert R.same(w.grad, want)
    assert R.same(b.grad, ops['dy'].double().sum(0, keepdim=True))
    ops = R.exact_operands(6, n, 8, 0, K, 32, n)
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    R.assert_exact(R.S_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0']), ref, ops['g'])
    assert R.same(_forward(ops, rb, K, n, 32, ops['bias'], ops['y0'], 'bias_acc', None), ref)
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'])
    assert R.same(_forward(ops, rb, K, n, 32, None, None, 'wide', None), ref)


# ------------------------------------------------------------------ 1x1
# (n_out, n_in, c1, c2, cout, mode)
ONE_BY_ONE = [(65, 65, 16, 0, 1, 'bias'), (700, 700, 96, 0, 3, 'plain'), (129, 200, 96, 0, 13, 'acc'), (513, 513, 96, 32, 20, 'bias_acc'), (4033, 4033, 320, 0, 32, 'plain'),
              (700, 700, 96, 0, 96, 'wide'), (1, 1, 16, 0, 128, 'bias'),
              (65537, 65537, 16, 0, 128, 'bias_acc'),          # 1025 tiles x 4 strips: two strips per wave
              (131073, 131073, 16, 0, 96, 'acc')]              # 2049 tiles x 3 strips: three strips per wave


# (the strips-per-wave forms exist in the streaming-GEMM kernel only: the two large cases do not run through the general kernel)
@pytest.mark.parametrize('n_out,n_in,c1,c2,cout,mode,general',
                         [pytest.param(*c, g, id='%d<-%d-%d+%d-%d-%s-%s' % (c + ('B2M_CONV_1X1=0' if g else 'gemm',)))
                          for g in (False, True) for c in ONE_BY_ONE if not (g and c[0] > 5000)])
def test_1x1_layer_is_the_rule_bit_for_bit(monkeypatch, n_out, n_in, c1, c2, cout, mode, general):
    from box2mask_amd import functional as F_
    if general:
        monkeypatch.setenv('B2M_CONV_1X1', '0')
        monkeypatch.setenv('B2M_WGRAD_PIPE_IDENT', '0')
    ops = R.exact_operands(7, n_in, c1, c2, 1, cout, n_out)
    bias = ops['bias'] if 'bias' in mode else None
    y0 = ops['y0'] if 'acc' in mode else None
    x1, x2 = ops['x1'], ops['x2']
    ref = R.conv_fwd(None, x1[:n_out], None if x2 is None else x2[:n_out], ops['w'], bias, y0)
    R.assert_exact(R.S_fwd(None, x1[:n_out], None if x2 is None else x2[:n_out], ops['w'], bias, y0), ref, ops['g'])
    y = _forward(ops, None, 1, n_out, cout, bias, y0, mode, None)
    assert R.same(y, ref), float((y.cpu().double() - ref).abs().max())
    dy = _dev(ops['dy'])
    if n_in == n_out:                                     # the data gradient of a 1x1 layer: dY W^T, per source
        for c0, c in ((0, c1), (c1, c2)):
            if c:
                want = R.conv_dgrad(None, ops['dy'], ops['w'], n_in, c0, c)
                R.assert_exact(R.S_dgrad(None, ops['dy'], ops['w'], n_in, c0, c), want, ops['g'])
                dx = F_.conv_raw(dy, None, F_.weight_pack(ops['w'].cuda(), True, False, c0, c), 1, None, None, n_in, c)
                assert R.same(dx, want)
    dw = ops['dw0'].cuda().clone()
    want = ops['dw0'].double()
    for x, ci0 in ((x1, 0), (x2, c1)):
        if x is not None:
            R.assert_exact(R.S_wgrad(None, x, ops['dy'], want, ci0), R.conv_wgrad(None, x, ops['dy'], want, ci0), 1.0)
            want = R.conv_wgrad(None, x, ops['dy'], want, ci0)
            F_.wgrad_raw(x.cuda(), dy, None, 1, dw, ci0, x.shape[1])
    assert R.same(dw, want), float((dw.cpu().double() - want).abs().max())


# ------------------------------------------------------------------ the inference epilogue
def _affine(x1, x2, w, rb, n_out, scale, shift, res, relu):
    """conv_affine, and whether the library fused the epilogue into the convolution."""
    from box2mask_amd import _lib, functional as F_
    seen = []

    def hook(name, args, meta):
        if name == 'b2m_conv_fwd_affine':
            return lambda: seen.append(args[-1]._obj.value)
        return None
    _lib.set_hook(hook)
    try:
        out = F_.conv_affine(x1, x2, w, rb, n_out, scale, shift, res, relu)
    finally:
        _lib.set_hook(None)
    torch.cuda.synchronize()
    return out, (seen[0] if seen else None)


@pytest.mark.parametrize('name,res,relu', [('L1', True, True), ('L3', False, True), ('L5', True, False), ('L8', True, True),
                                           ('L7', False, False), ('L12', True, True), ('L11', False, True), ('L14', True, True)])
def test_epilogue_is_the_rule_whatever_is_fused(monkeypatch, name, res, relu):
    table, K, n_out, n_in, c1, c2, cout, mode, view = LAYERS[name]
    ref = _layer_ref(name)
    ops, nbr = ref['ops'], ref['nbr']
    y64 = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'])
    want = R.epilogue(y64, ops['scale'], ops['shift'], ops['res'] if res else None, relu)
    w = ops['w'].cuda()
    for env in ({}, {'B2M_CONV_TARGET': '0'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out, fused = _affine(_dev(ops['x1']), _dev(ops['x2']), w, _rulebook(nbr, n_in), n_out, ops['scale'].cuda(), ops['shift'].cuda(),
                             ops['res'].cuda() if res else None, relu)
        print('%s %s: fused = %s' % (name, env, fused))
        assert R.same(out, want), float((out.cpu().double() - want).abs().max())
        if cout % 4:
            assert fused == 0, 'a vector epilogue on %d columns' % cout
        elif env:
            # un-split, the epilogue rides on the flow kernel: whole 16-channel chunks in pairs (conv_fwd_impl); an odd chunk count
            # (L14: 48 channels) runs the general kernel, which has no epilogue
            assert fused == (1 if (c1 + c2) % 32 == 0 else 0), 'un-split %d -> %d: fused = %s' % (c1 + c2, cout, fused)


@pytest.mark.parametrize('n_out,n_in,c1,c2,cout', [(65, 65, 16, 0, 32), (513, 600, 96, 32, 20), (700, 700, 96, 0, 13), (4033, 4033, 320, 0, 128)])
def test_epilogue_of_1x1_layers(n_out, n_in, c1, c2, cout):
    ops = R.exact_operands(8, n_in, c1, c2, 1, cout, n_out)
    x1, x2 = ops['x1'], ops['x2']
    y64 = R.conv_fwd(None, x1[:n_out], None if x2 is None else x2[:n_out], ops['w'])
    for res, relu in ((None, False), (ops['res'], True)):
        want = R.epilogue(y64, ops['scale'], ops['shift'], res, relu)
        out, fused = _affine(x1.cuda(), _dev(x2), ops['w'][0].cuda().contiguous(), None, n_out, ops['scale'].cuda(), ops['shift'].cuda(), _dev(res), relu)
        assert R.same(out, want)
        assert fused == (1 if cout % 4 == 0 else 0)


# ------------------------------------------------------------------ tile statistics
STATS_FORMS = {'unsplit': {'B2M_CONV_TARGET': '0'}, 'split4': {'B2M_CONV_TARGET': '512', 'B2M_CONV_CHUNKSPLIT': '0'},
               'split2': {'B2M_CONV_TARGET': '0', 'B2M_CONV_SPLIT2': '100000000'},
               'many_slices': {'B2M_CONV_TARGET': '100000', 'B2M_CONV_MAXSLICE': '16'}}


@pytest.mark.parametrize('form', sorted(STATS_FORMS))
@pytest.mark.parametrize('c1,c2,cout', [(32, 0, 64), (96, 32, 96)])
def test_tile_statistics_are_the_rule_exactly(monkeypatch, form, c1, c2, cout):
    """Both sums are fp64 on the device: exact on these operands (|y| <= 4096 g, so that y * y is exact even in fp32), including the
    partial last tile (4033 rows) and, un-split, on top of an accumulated y0."""
    from box2mask_amd import functional as F_
    for k, v in STATS_FORMS[form].items():
        monkeypatch.setenv(k, v)
    K, n = 27, 4033
    nbr = R.table('mixed', K, n, n, seed=2)
    rb = _rulebook(nbr, n)
    ops = R.exact_operands(2, n, c1, c2, K, cout, n, xmax=1, wmax=2, bmax=4)
    wp = F_.weight_pack(ops['w'].cuda())
    for acc in ((False, True) if form == 'unsplit' else (False,)):
        y0 = ops['y0'] if acc else None
        ref = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], y0)
        S_ = R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], y0)
        R.assert_exact(S_, ref, ops['g'])
        assert float(S_.max()) <= 4096 * ops['g']
        holder = []
        y = F_.conv_raw(_dev(ops['x1']), _dev(ops['x2']), wp, K, ops['bias'].cuda(), rb, n, cout,
                        out=y0.cuda().clone() if acc else None, accumulate=acc, tile_stats=holder)
        torch.cuda.synchronize()
        assert R.same(y, ref)
        if form == 'many_slices':
            assert holder == [], 'more than 4 slices: no workgroup owns a tile\'s sums'
            continue
        assert len(holder) == 1 and holder[0][1] == (n + 63) // 64
        assert torch.equal(holder[0][0].cpu(), R.tile_sums(ref)), 'tile sums differ from the rule'


# ------------------------------------------------------------------ strided and transposed maps from CoordinateManager
def _cells(children):
    """Coarse cells (0, 2i, 0, 0) with `children[i]` fine voxels each, in a shuffled row order."""
    rng = np.random.default_rng(len(children))
    rows = []
    for i, nch in enumerate(children):
        for j in rng.permutation(8)[:nch]:
            rows.append((0, 2 * i + (j & 1), (j >> 1) & 1, (j >> 2) & 1))
    c = np.array(rows, np.int32)
    return c[rng.permutation(len(c))]


def _grid30():
    rng = np.random.default_rng(30)
    occ = rng.random((2, 22, 20, 12)) < 0.3
    c = np.argwhere(occ).astype(np.int32)
    return c[rng.permutation(len(c))]


MAPS = {'1_child': lambda: _cells([1]), '2_children': lambda: _cells([2]), '8_children': lambda: _cells([8]),
        '65_cells': lambda: _cells([1 + (i * 5) % 8 for i in range(65)]), 'grid30': _grid30}
_maps = {}


def _map(name):
    """(manager, oracle tables with rows in the MANAGER's order: child[8, nc], up[8, nf])."""
    from box2mask_amd.sparse import CoordinateManager
    from oracle import sparse_ref as S
    if name not in _maps:
        fine = MAPS[name]()
        m = CoordinateManager(torch.from_numpy(fine))
        m.ensure_level(1)
        assert np.array_equal(m.coords[0].cpu().numpy(), fine)
        coarse_o, parent_o, koff = S.stride_coords(fine, 1)
        kg = S.pack_keys(m.coords[1].cpu().numpy()); ko = S.pack_keys(coarse_o)
        order = np.argsort(kg)
        to_dev = order[np.searchsorted(kg[order], ko)]               # oracle coarse row -> manager coarse row
        assert np.array_equal(kg[to_dev], ko) and len(kg) == len(ko)
        parent = to_dev[parent_o].astype(np.int32)
        _maps[name] = (m, S.child_table(parent, koff, len(kg)), S.up_table(parent, koff))
    return _maps[name]


MAP_ENVS = {'default': {}, 'scatter_form': {'B2M_CONV_UP_MIN_ITEMS': '1'}, 'no_scatter_form': {'B2M_CONV_UP': '0'},
            'wgrad_over_up_rulebook': {'B2M_CONV_UP_MIN_ITEMS': '1', 'B2M_WGRAD_UP': '0'}}


@pytest.mark.parametrize('env', sorted(MAP_ENVS))
@pytest.mark.parametrize('name,c1,c2,cout', [('1_child', 32, 0, 32), ('2_children', 32, 0, 96), ('8_children', 96, 32, 64),
                                             ('65_cells', 64, 0, 32), ('grid30', 96, 0, 96), ('grid30', 32, 32, 48)])
def test_strided_and_transposed_layers_are_the_rule_bit_for_bit(monkeypatch, name, c1, c2, cout, env):
    from box2mask_amd import functional as F_
    for k, v in MAP_ENVS[env].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('B2M_WGRAD_STREAM', '0')
    m, child, up = _map(name)
    nc, nf = child.shape[1], up.shape[1]
    for kind, nbr, n_out, n_in, rb_f, rb_b in (('down', child, nc, nf, m.rulebook_down(0), m.rulebook_up(0)),
                                                ('up', up, nf, nc, m.rulebook_up(0), m.rulebook_down(0))):
        ops = R.exact_operands(9, n_in, c1, c2, 8, cout, n_out)
        ref = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'])
        R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w']), ref, ops['g'])
        x1 = ops['x1'].cuda().requires_grad_(True)
        x2 = ops['x2'].cuda().requires_grad_(True) if c2 else None
        w = ops['w'].cuda().requires_grad_(True)
        y = F_.sparse_conv(x1, x2, w, None, rb_f, rb_b, False, n_out)
        y.backward(ops['dy'].cuda())
        torch.cuda.synchronize()
        assert R.same(y, ref), (kind, 'forward')
        dx = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in)
        R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n_in), dx, ops['g'])
        assert R.same(x1.grad, dx[:, :c1]), (kind, 'data gradient')
        if c2:
            assert R.same(x2.grad, dx[:, c1:]), (kind, 'data gradient of the second source')
        dw = R.conv_wgrad(nbr, R._cat(ops['x1'], ops['x2']), ops['dy'], torch.zeros_like(ops['w']))
        R.assert_exact(R.S_wgrad(nbr, R._cat(ops['x1'], ops['x2']), ops['dy'], torch.zeros_like(ops['w'])), dw, 1.0)
        assert R.same(w.grad, dw), (kind, 'weight gradient')
        # accumulate + bias through conv_raw on the same map
        ref = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'])
        R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0']), ref, ops['g'])
        assert R.same(_forward(ops, rb_f, 8, n_out, cout, ops['bias'], ops['y0'], 'bias_acc', None), ref), (kind, 'bias + accumulate')


# ------------------------------------------------------------------ weight gradient: block shapes
# (table, K, n_out, n_in, cin, cout, view of x)
WGRAD = [('mixed', 27, 129, 129, 16, 16, None), ('random', 27, 513, 513, 32, 32, None), ('mixed', 125, 65, 65, 8, 32, 'pitch16'),
         ('dense', 8, 129, 200, 32, 96, None), ('mixed', 27, 700, 700, 48, 48, None), ('random', 27, 4033, 4033, 64, 64, None),
         ('mixed', 27, 513, 513, 96, 96, None), ('random', 8, 65, 65, 128, 128, None), ('mixed', 27, 513, 513, 80, 32, None),
         ('mixed', 27, 4033, 4033, 80, 48, 'pitch128'), ('broadcast', 27, 129, 64, 48, 64, None), ('last_row', 27, 4033, 4033, 96, 16, None)]
WGRAD_ENVS = {'default': {}, 'plain': {'B2M_WGRAD_PIPE': '0'}, 'no_kpack': {'B2M_WGRAD_KPACK': '0'}, '64_tile_chunks': {'B2M_WGRAD_MIN_TILES': '64'},
              '64bit': {'B2M_WGRAD_FAST32': '0'}, 'deterministic': {'B2M_DETERMINISTIC': '1'}}


# (only layers of one or two blocks pack offsets: B2M_WGRAD_KPACK=0 runs on those)
@pytest.mark.parametrize('case,env', [pytest.param(c, e, id='%s-K%d-%d<-%d-%d-%d-%s-' % c + e) for e in sorted(WGRAD_ENVS) for c in WGRAD
                                      if not (e == 'no_kpack' and not (c[4] <= 32 and c[5] <= 96))])
def test_weight_gradient_block_shapes(monkeypatch, case, env):
    from box2mask_amd import functional as F_
    table, K, n_out, n_in, cin, cout, view = case
    for k, v in WGRAD_ENVS[env].items():
        monkeypatch.setenv(k, v)
    key = ('wgrad',) + case
    if key not in _refs:
        nbr = R.table(table, K, n_out, n_in, seed=4)
        ops = R.exact_operands(4, n_in, cin, 0, K, cout, n_out)
        want = R.conv_wgrad(nbr, ops['x1'], ops['dy'], ops['dw0'])
        R.assert_exact(R.S_wgrad(nbr, ops['x1'], ops['dy'], ops['dw0']), want, 1.0)
        _refs[key] = (nbr, ops, want)
    nbr, ops, want = _refs[key]
    rb = _rulebook(nbr, n_in)
    runs = []
    for _ in range(2 if env == 'deterministic' else 1):
        dw = ops['dw0'].cuda().clone()
        F_.wgrad_raw(_view(ops['x1'], view), ops['dy'].cuda(), rb, K, dw, 0, cin)
        assert R.same(dw, want), float((dw.cpu().double() - want).abs().max())
        runs.append(dw.cpu())
    assert all(torch.equal(r, runs[0]) for r in runs)


# ------------------------------------------------------------------ half kernels
WGRAD_FORMS = {'f16_mfma': {}, 'converted': {'B2M_WGRAD_TRH': '0'}, 'converted_plain': {'B2M_WGRAD_TRH': '0', 'B2M_WGRAD_PIPE': '0'}}
# (table, K, n_out, n_in, c1, c2, cout)
HALF = [('dense', 27, 1, 1, 32, 0, 32), ('mixed', 27, 65, 65, 96, 32, 96), ('random', 8, 513, 600, 96, 0, 256), ('mixed', 27, 4033, 4033, 32, 0, 96),
        ('centre', 27, 513, 513, 256, 0, 32), ('last_row', 27, 4033, 4033, 96, 0, 96), ('identity', 1, 4033, 4033, 96, 32, 32),
        ('broadcast', 27, 65, 40, 32, 0, 32)]


def _half_ops(seed, n_in, c1, c2, K, cout, n_out):
    return R.exact_operands(seed, n_in, c1, c2, K, cout, n_out, xmax=1, wmax=1, g=0.25, bmax=2)


# (the converted forms: one case per block shape)
@pytest.mark.parametrize('case,form', [pytest.param(c, f, id='%s-K%d-%d<-%d-%d+%d-%d-' % c + f) for f in sorted(WGRAD_FORMS) for c in HALF
                                       if f == 'f16_mfma' or c[0] in ('mixed', 'identity', 'random')])
def test_half_layer_is_the_rule_bit_for_bit(monkeypatch, case, form):
    from box2mask_amd import half_train as HT
    table, K, n_out, n_in, c1, c2, cout = case
    monkeypatch.setenv('B2M_WGRAD_STREAM', '0')
    for k, v in WGRAD_FORMS[form].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(HT, 'loss_scale', [1.0])
    HT.images.__init__()
    nbr = np.arange(n_out, dtype=np.int32).reshape(1, -1) if table == 'identity' else R.table(table, K, n_out, n_in, seed=12)
    ops = _half_ops(12, n_in, c1, c2, K, cout, n_out)
    g = ops['g']
    ref = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'])
    R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w']), ref, g)
    R.assert_half_exact(ref, g)
    rb = _rulebook(nbr, n_in)
    rev = R.has_reverse(nbr)
    rbr = _rulebook(R.reverse_table(nbr, n_in), n_out) if rev else rb
    x1 = ops['x1'].cuda().half().requires_grad_(rev)
    x2 = ops['x2'].cuda().half().requires_grad_(rev) if c2 else None
    w = ops['w'].cuda().requires_grad_(True)
    try:
        y = HT.conv(x1, x2, w, rb, rbr, False, n_out)
        y.backward(ops['dy'].cuda().half())
        torch.cuda.synchronize()
    finally:
        HT.images.__init__()
    assert y.dtype == torch.float16 and R.same(y, ref), 'forward'
    if rev:
        dx = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in)
        R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n_in), dx, g)
        R.assert_half_exact(dx, g)
        assert R.same(x1.grad, dx[:, :c1]), 'data gradient'
        if c2:
            assert R.same(x2.grad, dx[:, c1:]), 'data gradient of the second source'
    dw = R.conv_wgrad(nbr, R._cat(ops['x1'], ops['x2']), ops['dy'], torch.zeros_like(ops['w']))
    R.assert_exact(R.S_wgrad(nbr, R._cat(ops['x1'], ops['x2']), ops['dy'], torch.zeros_like(ops['w'])), dw, 1.0)
    assert w.grad.dtype == torch.float32 and R.same(w.grad, dw), 'weight gradient'


@pytest.mark.parametrize('case', HALF[:4] + HALF[6:7], ids=lambda c: '%s-K%d-%d<-%d-%d+%d-%d' % c)
def test_half_inference_layer_is_the_rule_bit_for_bit(case):
    """conv_affine_h / weight_pack_h: with and without the epilogue (scale, shift, residual, ReLU)."""
    from box2mask_amd import functional as F_
    table, K, n_out, n_in, c1, c2, cout = case
    nbr = np.arange(n_out, dtype=np.int32).reshape(1, -1) if table == 'identity' else R.table(table, K, n_out, n_in, seed=12)
    ops = _half_ops(13, n_in, c1, c2, K, cout, n_out)
    rb = _rulebook(nbr, n_in)
    y64 = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'])
    R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w']), y64, ops['g'])
    w = ops['w'].cuda()
    x1 = ops['x1'].cuda().half(); x2 = ops['x2'].cuda().half() if c2 else None
    y = F_.conv_affine_h(x1, x2, w, rb, n_out)
    R.assert_half_exact(y64, ops['g'])
    assert R.same(y, y64)
    want = R.epilogue(y64, ops['scale'], ops['shift'], ops['res'], True)
    R.assert_half_exact(want, ops['g'] / 2)
    y = F_.conv_affine_h(x1, x2, w, rb, n_out, ops['scale'].cuda(), ops['shift'].cuda(), ops['res'].cuda().half(), True)
    assert R.same(y, want)


# ------------------------------------------------------------------ the arithmetic family: full-mantissa operands, short sums
def _report(family, r):
    print('conv_rule ratio %-28s %.3f' % (family, r))


@pytest.mark.parametrize('n', [65, 4033])
@pytest.mark.parametrize('family,K,cin,cout,two,env', [
    ('general', 27, 16, 32, True, {}), ('flow', 27, 32, 48, True, {}), ('flow_unsplit', 27, 32, 32, False, {'B2M_CONV_TARGET': '0'}),
    ('stem', 125, 8, 32, True, {'B2M_CONV_TARGET': '0'}), ('general_k8', 8, 16, 16, True, {})])
def test_forward_arithmetic_stays_inside_the_bound(monkeypatch, family, K, cin, cout, two, env, n):
    from box2mask_amd import functional as F_
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nbr = R.two_neighbour_table(K, n, n, seed=6) if two and cin * 2 <= 64 else R.table('centre', K, n, n, seed=6)
    ops = R.full_operands(6, n, cin, 0, K, cout, n)
    T = R.terms_fwd(nbr, cin)
    assert float(T.max()) <= 64
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    bnd = R.bound(T, R.S_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0']))
    y = _forward(ops, _rulebook(nbr, n), K, n, cout, ops['bias'], ops['y0'], 'bias_acc', None)
    ok, r = R.inside(y, ref, bnd)
    _report('%s rows %d' % (family, n), r)
    assert ok, r
    # the data gradient (the same kernels over the reverse table); where two neighbours give an input row more than 64 products
    # (cout 48), over the centre offset alone
    if float(R.terms_dgrad(nbr, cout, n).max()) > 64:
        nbr = R.table('centre', K, n, n, seed=6)
    refd = R.conv_dgrad(nbr, ops['dy'], ops['w'], n)
    Td = R.terms_dgrad(nbr, cout, n)
    assert float(Td.max()) <= 64
    dx = F_.conv_raw(ops['dy'].cuda(), None, F_.weight_pack(ops['w'].cuda(), True, False, 0, cin), K, None,
                     _rulebook(R.reverse_table(nbr, n), n), n, cin)
    ok, r = R.inside(dx, refd, R.bound(Td, R.S_dgrad(nbr, ops['dy'], ops['w'], n)))
    _report('%s dgrad rows %d' % (family, n), r)
    assert ok, r


@pytest.mark.parametrize('n', [65, 4033])
@pytest.mark.parametrize('cin,cout', [(16, 32), (32, 13)])
def test_1x1_arithmetic_stays_inside_the_bound(n, cin, cout):
    ops = R.full_operands(7, n, cin, 0, 1, cout, n)
    ref = R.conv_fwd(None, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    bnd = R.bound(R.terms_fwd(None, cin, n), R.S_fwd(None, ops['x1'], None, ops['w'], ops['bias'], ops['y0']))
    ok, r = R.inside(_forward(ops, None, 1, n, cout, ops['bias'], ops['y0'], 'bias_acc', None), ref, bnd)
    _report('1x1 %d->%d rows %d' % (cin, cout, n), r)
    assert ok, r


@pytest.mark.parametrize('name', ['65_cells', 'grid30'])
def test_scatter_form_arithmetic_stays_inside_the_bound(monkeypatch, name):
    monkeypatch.setenv('B2M_CONV_UP_MIN_ITEMS', '1')
    m, child, up = _map(name)
    nc, nf = child.shape[1], up.shape[1]
    ops = R.full_operands(8, nc, 32, 0, 8, 32, nf)
    T = R.terms_fwd(up, 32)
    assert float(T.max()) <= 64
    ref = R.conv_fwd(up, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    bnd = R.bound(T, R.S_fwd(up, ops['x1'], None, ops['w'], ops['bias'], ops['y0']))
    ok, r = R.inside(_forward(ops, m.rulebook_up(0), 8, nf, 32, ops['bias'], ops['y0'], 'bias_acc', None), ref, bnd)
    _report('scatter-form up %s' % name, r)
    assert ok, r


@pytest.mark.parametrize('n', [65, 4033])
@pytest.mark.parametrize('family,K,cin,cout,env', [('wgrad_pipelined', 27, 32, 32, {}), ('wgrad_plain', 27, 32, 32, {'B2M_WGRAD_PIPE': '0'}),
                                                   ('wgrad_single_accumulator', 27, 16, 16, {}), ('wgrad_deterministic', 8, 32, 16, {'B2M_DETERMINISTIC': '1'})])
def test_weight_gradient_arithmetic_stays_inside_the_bound(monkeypatch, family, K, cin, cout, env, n):
    from box2mask_amd import functional as F_
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nbr = R.few_pairs_table(K, n, n, 48, seed=6)
    ops = R.full_operands(9, n, cin, 0, K, cout, n)
    T = R.terms_wgrad(nbr)
    assert float(T.max()) <= 64
    ref = R.conv_wgrad(nbr, ops['x1'], ops['dy'], ops['dw0'])
    # (n = T + 16 as everywhere: a product in a tile chunk's partial sum of t pairs meets t roundings there and one add per partial
    # sum, and every further partial sum shortens a chain by at least one pair)
    bnd = R.bound(T, R.S_wgrad(nbr, ops['x1'], ops['dy'], ops['dw0']))
    dw = ops['dw0'].cuda().clone()
    F_.wgrad_raw(ops['x1'].cuda(), ops['dy'].cuda(), _rulebook(nbr, n), K, dw, 0, cin)
    ok, r = R.inside(dw, ref, bnd)
    _report('%s rows %d' % (family, n), r)
    assert ok, r


@pytest.mark.parametrize('cout', [3, 13])
def test_narrow_weight_gradient_arithmetic_stays_inside_the_bound(cout):
    """wgrad_narrow_kernel sums over ALL rows of a 1x1 layer: T = n_out, so the short-sum family stops at 63 rows here."""
    from box2mask_amd import functional as F_
    n, cin = 63, 32
    ops = R.full_operands(10, n, cin, 0, 1, cout, n)
    ref = R.conv_wgrad(None, ops['x1'], ops['dy'], ops['dw0'])
    T = torch.full((1, 1, 1), float(n), dtype=torch.float64)
    assert float(T.max()) <= 64
    dw = ops['dw0'].cuda().clone()
    F_.wgrad_raw(ops['x1'].cuda(), ops['dy'].cuda(), None, 1, dw, 0, cin)
    ok, r = R.inside(dw, ref, R.bound(T, R.S_wgrad(None, ops['x1'], ops['dy'], ops['dw0'])))
    _report('wgrad_narrow cout %d' % cout, r)
    assert ok, r


@pytest.mark.parametrize('n', [65, 4033])
def test_half_arithmetic_stays_inside_the_bound(monkeypatch, n):
    """One short-sum full-mantissa case per half kernel: operands rounded to binary16 first (they ARE the operands), the result
    held to the fp32 bound + one half rounding of the result.  Forward and data gradient on the two-neighbour table (T <= 64), the
    weight gradient on a table with 48 pairs per offset."""
    from box2mask_amd import half_train as HT
    monkeypatch.setenv('B2M_WGRAD_STREAM', '0')
    monkeypatch.setattr(HT, 'loss_scale', [1.0])
    K, cin, cout = 27, 32, 32
    ops = R.half_of(R.full_operands(11, n, cin, 0, K, cout, n))
    ops['x1'] = ops['x1'] / 8; ops['dy'] = ops['dy'] / 8            # (|y| < 65504: 64 terms of at most 2^12 / 8 each)

    def run(nbr):
        HT.images.__init__()
        x = ops['x1'].cuda().half().requires_grad_(True); w = ops['w'].cuda().requires_grad_(True)
        assert torch.equal(x.detach().float().cpu(), ops['x1'])
        try:
            y = HT.conv(x, None, w, _rulebook(nbr, n), _rulebook(R.reverse_table(nbr, n), n), False, n)
            y.backward(ops['dy'].cuda().half())
            torch.cuda.synchronize()
        finally:
            HT.images.__init__()
        return y, x.grad, w.grad
    nbr = R.two_neighbour_table(K, n, n, seed=3)
    y, dx, _ = run(nbr)
    T = R.terms_fwd(nbr, cin)
    assert float(T.max()) <= 64
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'])
    ok, r = R.inside(y.float(), ref, R.bound_half(T, R.S_fwd(nbr, ops['x1'], None, ops['w']), ref))
    _report('half forward rows %d' % n, r)
    assert ok, r
    refd = R.conv_dgrad(nbr, ops['dy'], ops['w'], n)
    Td = R.terms_dgrad(nbr, cout, n)
    assert float(Td.max()) <= 64
    ok, r = R.inside(dx.float(), refd, R.bound_half(Td, R.S_dgrad(nbr, ops['dy'], ops['w'], n), refd))
    _report('half dgrad rows %d' % n, r)
    assert ok, r
    nbr = R.few_pairs_table(K, n, n, 48, seed=3)
    _, _, dw = run(nbr)
    zero = torch.zeros(K, cin, cout)
    refw = R.conv_wgrad(nbr, ops['x1'], ops['dy'], zero)
    Tw = R.terms_wgrad(nbr)
    assert float(Tw.max()) <= 64
    ok, r = R.inside(dw, refw, R.bound(Tw, R.S_wgrad(nbr, ops['x1'], ops['dy'], zero)))
    _report('half wgrad rows %d' % n, r)
    assert ok, r


# ------------------------------------------------------------------ empty maps
def test_empty_outputs_and_inputs(monkeypatch):
    """n_out = 0: every entry returns after its scalar-argument checks whatever the (empty) tensors' pointers are, n_in = 0 included.
    n_in = 0 with output rows: the weight gradient has no pairs and leaves dW alone; the forward entry refuses (its kernels are
    given a row to read) -- with a message, not a fault."""
    from box2mask_amd import _lib, functional as F_, half_train as HT
    monkeypatch.setenv('B2M_WGRAD_STREAM', '0')
    monkeypatch.setattr(HT, 'loss_scale', [1.0])
    K, cin, cout = 27, 32, 32
    w = R.exact_operands(0, 1, cin, 0, K, cout, 1)['w'].cuda()
    wp = F_.weight_pack(w)
    empty = lambda c, dt=torch.float32: torch.empty((0, c), dtype=dt, device='cuda')
    for n_in in (0, 5):
        rb = _rulebook(np.zeros((K, 0), np.int32), n_in)
        x = torch.ones((n_in, cin), device='cuda')
        assert tuple(F_.conv_raw(x, None, wp, K, None, rb, 0, cout).shape) == (0, cout)
        assert tuple(F_.conv_raw(x, None, wp, K, None, rb, 0, cout, tile_stats=[]).shape) == (0, cout)
        assert tuple(F_.conv_affine(x, None, w, rb, 0, torch.ones(cout, device='cuda'), torch.zeros(cout, device='cuda')).shape) == (0, cout)
        assert tuple(F_.conv_raw(x, None, F_.weight_pack(w[:1].contiguous()), 1, None, None, 0, cout).shape) == (0, cout)
        dw = torch.full((K, cin, cout), 3.0, device='cuda')
        F_.wgrad_raw(x, empty(cout), rb, K, dw, 0, cin)
        assert bool((dw == 3.0).all())
        assert tuple(F_.conv_affine_h(x.half(), None, w, rb, 0).shape) == (0, cout)
        if n_in:
            continue
        # the autograd operators on an empty map: empty result, zero weight gradient, empty data gradient
        for op, xx in ((F_.sparse_conv, x.clone().requires_grad_(True)), (HT.conv, x.half().requires_grad_(True))):
            ww = w.clone().requires_grad_(True)
            y = op(xx, None, ww, None, rb, rb, False, 0) if op is F_.sparse_conv else op(xx, None, ww, rb, rb, False, 0)
            y.backward(torch.empty_like(y))
            torch.cuda.synchronize()
            assert tuple(y.shape) == (0, cout) and not bool(ww.grad.any()) and tuple(xx.grad.shape) == (0, cin)
    # the C entries that the Python wrappers guard themselves, called directly on an empty map with address-less tensors
    rb = _rulebook(np.zeros((K, 0), np.int32), 0)
    e16, eh = empty(cin), empty(cin, torch.float16)
    image = F_.weight_pack_h(w, cin, 0)
    F_._call('b2m_conv_fwd_h', eh.data_ptr(), cin, cin, None, 0, 0, 0, image.data_ptr(), K, rb.rb_in.data_ptr(), rb.rb_out.data_ptr(),
             rb.rb_cnt.data_ptr(), 0, eh.data_ptr(), cout, cout, None, None, None, 0, 0)
    ran = ctypes.c_int32(0)
    F_._call('b2m_conv_up', e16.data_ptr(), cin, cin, None, 0, 0, 0, wp.data_ptr(), K, None, rb.rb_in.data_ptr(), rb.rb_out.data_ptr(),
             rb.rb_cnt.data_ptr(), e16.data_ptr(), cout, cout, 0, 0, None, None, None, 0, 0, ctypes.byref(ran))
    assert ran.value == 1
    fused = ctypes.c_int32(0)
    one = torch.ones(cout, device='cuda')
    F_._call('b2m_conv_fwd_affine', e16.data_ptr(), cin, cin, None, 0, 0, 0, wp.data_ptr(), K, rb.rb_in.data_ptr(), rb.rb_out.data_ptr(),
             rb.rb_cnt.data_ptr(), 0, e16.data_ptr(), cout, cout, one.data_ptr(), one.data_ptr(), None, 0, 0, ctypes.byref(fused))
    with pytest.raises(_lib.B2MError, match='channels must be multiples of 16'):      # ... behind the scalar checks, not in front of them
        F_._call('b2m_conv_fwd_h', eh.data_ptr(), 20, 20, None, 0, 0, 0, image.data_ptr(), K, rb.rb_in.data_ptr(), rb.rb_out.data_ptr(),
                 rb.rb_cnt.data_ptr(), 0, eh.data_ptr(), cout, cout, None, None, None, 0, 0)
    # output rows without input rows
    rb = _rulebook(np.full((K, 70), -1, np.int32), 0)
    dw = torch.full((K, cin, cout), 3.0, device='cuda')
    F_.wgrad_raw(empty(cin), torch.ones((70, cout), device='cuda'), rb, K, dw, 0, cin)
    assert bool((dw == 3.0).all())
    with pytest.raises(_lib.B2MError, match='n_in'):
        F_.conv_raw(empty(cin), None, wp, K, None, rb, 70, cout)


def test_per_element_apply_equals_the_vector_kernel():
    """b2m_bn_apply behind a convolution that did not fuse: a width or row pitch without 16-byte column groups takes one element per
    thread -- the same fmaf, residual add and ReLU, hence the same bits as the vector kernel on full-mantissa numbers."""
    from box2mask_amd import functional as F_
    n, c = 4033, 52
    ops = R.full_operands(14, n, c, 0, 1, c, n)
    x, res = ops['x1'].cuda(), ops['dy'].cuda()
    scale, shift = ops['bias'].cuda().reshape(-1), ops['w'][0, 0].cuda().contiguous()
    y_vec = torch.empty_like(x)
    F_._call('b2m_bn_apply', x.data_ptr(), c, n, c, scale.data_ptr(), shift.data_ptr(), res.data_ptr(), c, 1, y_vec.data_ptr(), c)
    xp = _view(ops['x1'], 'odd_pitch')
    y_el = torch.full((n, c + 3), -7.0, device='cuda')
    F_._call('b2m_bn_apply', xp.data_ptr(), xp.stride(0), n, c, scale.data_ptr(), shift.data_ptr(), res.data_ptr(), c, 1, y_el.data_ptr(), c + 3)
    torch.cuda.synchronize()
    assert torch.equal(y_el[:, :c], y_vec) and bool((y_el[:, c:] == -7.0).all())
    want = R.epilogue(ops['x1'], ops['bias'].reshape(-1), ops['w'][0, 0], ops['dy'], True)
    bnd = 3 * R.U32 * (ops['x1'].double() * ops['bias'].double().reshape(1, -1)).abs() + 3 * R.U32 * (ops['w'][0, 0].double().abs() + ops['dy'].double().abs())
    assert bool(((y_vec.cpu().double() - want).abs() <= bnd).all())       # (two roundings: the fmaf, the add)
