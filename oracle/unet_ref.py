"""ORACLE (test infrastructure; never imported by the product).

CPU restatement of SelectionNet.forward (/root/reference/models/detection_net.py:234-364) and of
BasicBlock.forward (/root/reference/models/resnet.py:70-83) on top of oracle/sparse_ref.py, written
as a pure function of a state dict with the reference's parameter names, so it can be
run against the product's weights.  torch CPU autograd provides the backward pass.

PARITY UNPINNED at the sparse-engine level (see the header of oracle/sparse_ref.py): the layer
schedule, channel plan and head structure follow the reference source line by line, but the numeric
behaviour of each sparse operator is pinned only by the independent checks in
tests/test_oracle_sparse.py, not by MinkowskiEngine itself.
"""
from __future__ import annotations

import torch

from . import sparse_ref as S


def _bn(p, name, x, training, stats_out=None):
    return S.batch_norm(x, p[name + '.bn.weight'], p[name + '.bn.bias'],
                        p[name + '.bn.running_mean'].clone(), p[name + '.bn.running_var'].clone(), training)


def _block(p, name, x, nbr, training, st=None, inject=None):
    """BasicBlock (resnet.py:70-83): conv3-BN-ReLU-conv3-BN (+1x1conv-BN residual) add ReLU.
    st (a sparse_ref.HalfStorage): the block runs in the binary16 region -- see `forward`."""
    if st is not None:
        return _block_stored(p, name, x, nbr, training, st, inject or {})
    out = S.conv_nbr(x, p[name + '.conv1.kernel'], nbr)
    out = torch.relu(_bn(p, name + '.norm1', out, training))
    out = S.conv_nbr(out, p[name + '.conv2.kernel'], nbr)
    out = _bn(p, name + '.norm2', out, training)
    if (name + '.downsample.0.kernel') in p:
        res = S.conv_nbr(x, p[name + '.downsample.0.kernel'], None)
        res = _bn(p, name + '.downsample.1', res, training)
    else:
        res = x
    return torch.relu(out + res)


def _block_stored(p, name, x, nbr, training, st, inject):
    """The block as box2mask_amd/resnet.py::BasicBlock.forward runs it on binary16 tensors (half_train.py).  Every convolution
    output and every BatchNorm output (after the residual add and the ReLU) is a storage point; the statistics are those of the
    ROUNDED convolution output.  Backward: a storage point rounds the gradient that arrives at it, which is
      * at a convolution output: the BatchNorm's dx;
      * at the block's input (the storage point of whoever produced x): conv1's data gradient PLUS the gradient of x's other
        consumer (residual / shortcut), summed un-rounded and rounded once -- the pass-through of _ConvH's epilogue;
      * the shortcut convolution's data gradient is a tensor of its own on the device, rounded before it enters that sum:
        `grad_only` on its input.  (dres of the fused BatchNorm is dy under the mask: no rounding of its own.)
    Every convolution multiplies with the binary16 image of its weights (`st.weight`).
    inject: the deliberate mistakes of tests/test_half_oracle_rule.py, {kind: block name}."""
    out = st.point(S.conv_nbr(x, st.weight(p[name + '.conv1.kernel']), nbr), 'conv')
    out = st.point(torch.relu(_bn(p, name + '.norm1', out, training)), 'bn')
    out = st.point(S.conv_nbr(out, st.weight(p[name + '.conv2.kernel']), nbr), 'conv')
    out = _bn(p, name + '.norm2', out, training)
    other = x.detach() if inject.get('drop_passthrough') == name else x
    if (name + '.downsample.0.kernel') in p:
        res = st.point(S.conv_nbr(st.grad_only(other), st.weight(p[name + '.downsample.0.kernel']), None), 'conv')
        res = st.point(_bn(p, name + '.downsample.1', res, training), 'bn')
    else:
        res = other
    if inject.get('drop_dres') == name:
        res = res.detach()
    pre = out + res
    y = torch.relu(pre)
    if inject.get('mask_before_add') == name:          # the forward value stays; the BACKWARD takes its mask from BN(x) alone
        y = y.detach() + (pre - pre.detach()) * (out.detach() > 0).to(out.dtype)
    return st.point(y, 'bn')


def _layer(p, name, x, nbr, training, n_blocks, st=None, inject=None):
    for b in range(n_blocks):
        x = _block(p, '%s.%d' % (name, b), x, nbr, training, st, inject)
    return x


def _head(p, name, x, training):
    """mlp_head (detection_net.py:170-194): conv1x1(+bias)-ReLU-BN, conv1x1-ReLU-BN, conv1x1."""
    x = torch.relu(S.conv_nbr(x, p[name + '.0.kernel'], None, p[name + '.0.bias']))
    x = _bn(p, name + '.2', x, training)
    x = torch.relu(S.conv_nbr(x, p[name + '.3.kernel'], None, p[name + '.3.bias']))
    x = _bn(p, name + '.5', x, training)
    return S.conv_nbr(x, p[name + '.6.kernel'], None, p[name + '.6.bias'])


HALF_LEVELS = 3       # half_train.py: the levels 0 ... 3 (tensor strides 1 ... 8) live in binary16

HEAD_ATTR = {'mlp_offsets': 'mlp_offsets', 'mlp_bounds': 'mlp_bounds', 'mlp_bb_scores': 'mlp_score',
             'mlp_center_scores': 'mlp_center_score', 'mlp_semantics': 'mlp_semantics',
             'mlp_per_vox_semantics': 'mlp_per_vox_semantics'}


def forward(p, coords, feats, pooling_ids, cfg, training=True, hier: S.Hierarchy | None = None, n_segments=None,
            return_trunk=False, trace=None, storage=None, loss_scale=1024.0, inject=None, tap=None):
    """p: dict name -> CPU tensor (the product's state_dict moved to the CPU).  Returns head -> tensor.

    storage=None: every tensor in the caller's dtype (nothing below is touched).
    storage='half' (or a sparse_ref.HalfStorage, to read its counters afterwards): the storage rule of the half-precision
    training pass, box2mask_amd/half_train.py as composed by nn.py, resnet.py::BasicBlock.forward and
    detection_net.py::SelectionNet.forward -- profiles/half_oracle_rule.md has the placement table:
      * the stem (conv0p1s1 + bn0) un-rounded; a storage point behind it (`to_half`);
      * every convolution output and every BatchNorm output (after residual add and ReLU) of the levels at tensor strides 1 ... 8
        -- conv1p1s2 ... block3, block5 ... block8 with their transposed layers -- is a storage point;
      * every convolution there multiplies with the binary16 IMAGE of its fp32 master weights, forward and data gradient
        (half_train._HalfImages); the weight gradient is the image's, un-rounded;
      * un-rounded across `to_float` into conv4p8s2 and into the pooling; strides >= 16, pooling and heads un-rounded; the
        output of convtr4p16s2 + bntr4 (fp32) is rounded at its `to_half`;
      * backward: a storage point rounds the gradient arriving at it as half(g * loss_scale) / loss_scale; `grad_only` does so
        where the device writes a half gradient of its own in front of a sum -- at both `to_float`s, on the skip branch of every
        ME.cat (block5 ... block8's conv1 writes the skip's gradient, the encoder's strided convolution then adds its own in its
        epilogue), on the input of a shortcut convolution.  Parameter gradients are never rounded.
    inject: {kind: layer name} -- the deliberate mistakes of tests/test_half_oracle_rule.py (storage='half' only).
    tap: callable (name, tensor) -> tensor applied at every traced point after `trace` took the tensor; the network goes on with
    what it returns (tests/_half_rule.py puts another pass's value and gradient there, to compare segment by segment)."""
    h = hier if hier is not None else S.Hierarchy(coords)
    L = cfg.layers
    x = feats
    st = None
    if storage is not None:
        st = storage if isinstance(storage, S.HalfStorage) else S.HalfStorage(loss_scale)
        assert isinstance(storage, S.HalfStorage) or storage == 'half', storage
    inject = inject or {}
    assert st is not None or not inject

    def cbr(conv, bn, x, nbr, st=None):
        if st is not None:
            y = S.conv_nbr(x, st.weight(p[conv + '.kernel']), nbr)
            return st.point(torch.relu(_bn(p, bn, st.point(y, 'conv'), training)), 'bn')
        y = S.conv_nbr(x, p[conv + '.kernel'], nbr)
        return torch.relu(_bn(p, bn, y, training))

    def T(name, t):
        if trace is not None:
            trace[name] = t
        return t if tap is None else tap(name, t)

    out_p1 = T('out_p1', cbr('conv0p1s1', 'bn0', x, h.k_first()))
    if st is not None:
        out_p1 = st.point(out_p1, 'to_half')
    enc = [out_p1]
    names = [('conv1p1s2', 'bn1', 'block1'), ('conv2p2s2', 'bn2', 'block2'), ('conv3p4s2', 'bn3', 'block3'),
             ('conv4p8s2', 'bn4', 'block4'), ('added_conv1p16s2', 'added_bn1', 'added_block1'),
             ('added_conv2p32s2', 'added_bn2', 'added_block2'), ('added_conv3p64s2', 'added_bn3', 'added_block3')]
    out = out_p1
    for l, (c, b, blk) in enumerate(names):          # level l -> l+1
        sl = st if l + 1 <= HALF_LEVELS else None    # the half region: levels 0 ... 3 (tensor strides 1 ... 8)
        if st is not None and sl is None and l == HALF_LEVELS:
            out = st.grad_only(out)                  # `to_float` in front of conv4p8s2: the gradient enters the region here
        out = T('down%d' % (l + 1), cbr(c, b, out, h.down(l), sl))
        out = T(blk, _layer(p, blk, out, h.k3(l + 1), training, L, sl, inject))
        enc.append(out)
    ups = [('added_convtr4p128s2', 'added_bntr4', 'added_block4'), ('added_convtr5p64s2', 'added_bntr5', 'added_block5'),
           ('added_convtr6p32s2', 'added_bntr6', 'added_block6'), ('convtr4p16s2', 'bntr4', 'block5'),
           ('convtr5p8s2', 'bntr5', 'block6'), ('convtr6p4s2', 'bntr6', 'block7'), ('convtr7p2s2', 'bntr7', 'block8')]
    for j, (c, b, blk) in enumerate(ups):            # level 7-j -> 6-j
        l = 6 - j
        sl = st if l <= HALF_LEVELS else None
        # (the transposed layer onto level 3 reads fp32 rows of level 4: it runs un-rounded and its result meets `to_half`)
        out = cbr(c, b, out, h.up(l), sl if l < HALF_LEVELS else None)
        skip = enc[l]
        if sl is not None:
            if l == HALF_LEVELS:
                if inject.get('scale_twice'):
                    out = S._ScaleGrad.apply(out, st.loss_scale)
                out = st.point(out, 'to_half')
            skip = st.grad_only(skip)
        out = T('up%d' % l, out)
        out = torch.cat([out, skip], 1)              # ME.cat(upsampled, skip): detection_net.py:286-336
        out = T(blk, _layer(p, blk, out, h.k3(l), training, L, sl, inject))
    if st is not None:
        out = st.grad_only(out)                      # `to_float` in front of the pooling
    trunk = out
    outputs = {}
    per_vox = any('per_vox' in hd for hd in cfg.network_heads)
    if per_vox:
        outputs['vox_feats'] = trunk
    if cfg.do_segment_pooling:
        ids = torch.as_tensor(pooling_ids).long()
        n_seg = int(ids.max()) + 1 if n_segments is None else n_segments
        out = S.segment_pool(out, ids, n_seg, 'max' if cfg.max_pool_segments_detection_net else 'avg')
    for hd in cfg.network_heads:
        src = trunk if (per_vox and 'per_vox' in hd) else out
        y = _head(p, HEAD_ATTR[hd], src, training)
        if cfg.mlp_bounds_relu and hd == cfg.mlp_bounds:
            y = torch.relu(y)
        outputs[hd] = y
    if return_trunk:
        outputs['_trunk'] = trunk
    return outputs
