"""The half-precision training pass of the device (box2mask_amd/half_train.py as nn.py, resnet.py and detection_net.py compose it)
against the fp64 oracle under the same storage rule: oracle/unet_ref.py forward(storage='half') rounds to binary16 exactly where the
device keeps a tensor in HBM as half (activations, gradients, the weight images) and sums in fp64 (profiles/half_oracle_rule.md; tests/test_half_oracle_rule.py checks the rule
itself on the CPU).

One device pass with the kernels' own ReLU path, its decisions recorded; then on the CPU, all with those decisions replayed:
  rule       the fp64 oracle under the storage rule, from the inputs;
  yardstick  the same call in fp32 -- no device code: what a correct half-storage pass whose sums are not fp64 shows against the rule;
  two forced passes of the fp64 rule, with the device's / the yardstick's value and gradient in place at every traced point
  (tests/_half_rule.py): the same comparison stretch by stretch.
Whole network every quantity of the device -- heads, the 29 traced tensors, the 283 parameter gradients, the cosine of the gradient
vector -- may be at most 4 x what the yardstick shows for the same quantity; per stretch its outputs, the gradient it sends back and its
parameter gradients are bounded from the yardstick's figures as _half_rule.segment_bounds says.  Both columns are printed.

Measured on the MI355X (profiles/half_oracle_rule.md has the tables): whole network the device is at 0.18 ... 0.47 of its bounds (heads
4.3e-2 against a yardstick of 4.9e-2, worst parameter gradient 1.4e-1 against 2.1e-1), stretch by stretch at 0.25 ... 0.37 (worst
parameter gradient 8.1e-4 against 8.0e-4).  A first draft of the rule without the binary16 weight images put six BatchNorm weights
8 ... 30 x past the yardstick stretch by stretch and one head 7 x past it whole network.

(Four oracle passes of 16 scenes: about the cost of the three 8-scene passes of test_network_forward_backward_matches_oracle plus
one.  16 scenes because 8 saturate binary16 under the loss scale 1024; the fourth pass because the whole-network yardstick is too
wide to see a 2 % error and the stretch-by-stretch comparison needs its own -- profiles/half_oracle_rule.md has the figures.)"""
import contextlib
import os

import numpy as np
import pytest
import torch

import _half_rule as R
from test_gpu_half_train import WGRAD_FORMS

pytestmark = pytest.mark.gpu

ENV = {'B2M_DETERMINISTIC': '1', 'B2M_BN_PAIR': '0'}


@contextlib.contextmanager
def _env(values):
    """B2M_* switches for the duration (the library caches them: reloaded on the way in and out), HT.images started over."""
    from box2mask_amd import _lib, half_train as HT
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    _lib.reload_env()
    images = HT.images
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.reload_env()
        HT.images = images
        HT.images.__init__()


class _Decisions:
    """The ReLU decisions of a device pass in call order -- F_.batch_norm / F_.relu as tests/_parity.py::MaskRecorder takes them, and
    half_train.batch_norm (whose rows are those of the one level of the half region with that many rows).  record: the kernels' own
    ReLU runs and y > 0 is kept.  replay: the layer runs without its ReLU and the result is multiplied by the recorded mask, as
    test_half_training_pass_against_the_fp32_pass does."""

    def __init__(self, replay=None):
        self.masks = [] if replay is None else replay        # [(level or None for pooled rows or ('rows', n), mask)]
        self.replaying, self.idx = replay is not None, 0

    def take(self, key, y):
        if not self.replaying:
            self.masks.append((key, y.detach() > 0))
            return None
        m = self.masks[self.idx][1]
        self.idx += 1
        assert m.shape == y.shape
        return m

    @contextlib.contextmanager
    def installed(self):
        from box2mask_amd import functional as F_, half_train as HT
        bn32, bn16, relu0 = F_.batch_norm, HT.batch_norm, F_.relu
        rp = self.replaying

        def p_bn32(x, gamma, beta, rm, rv, training, momentum=0.1, eps=1e-5, residual=None, relu=False, sync=False, count_key=None):
            y = bn32(x, gamma, beta, rm, rv, training, momentum, eps, residual, relu and not rp, sync, count_key)
            if not relu:
                return y
            m = self.take(count_key[2] if count_key[0] == 'level' else None, y)
            return y * m.to(y.dtype) if rp else y

        def p_bn16(x, gamma, beta, rm, rv, momentum, eps, residual=None, relu=False, sync=False):
            y = bn16(x, gamma, beta, rm, rv, momentum, eps, residual, relu and not rp, sync)
            if not relu:
                return y
            m = self.take(('rows', x.shape[0]), y)
            return y * m.to(y.dtype) if rp else y

        def p_relu(x):
            if rp:
                return x * self.take(None, x).to(x.dtype)
            y = relu0(x)
            self.take(None, y)
            return y
        F_.batch_norm, HT.batch_norm, F_.relu = p_bn32, p_bn16, p_relu
        try:
            yield self
        finally:
            F_.batch_norm, HT.batch_norm, F_.relu = bn32, bn16, relu0

    def in_oracle_order(self, to_gpu, hier, n_seg):
        half_level = {hier.n(l): l for l in range(4)}
        assert len(half_level) == 4
        out = []
        for key, m in self.masks:
            level = half_level[key[1]] if isinstance(key, tuple) else key
            m = m.cpu()
            assert m.shape[0] == (n_seg if level is None else hier.n(level))
            out.append(m if level is None else m[to_gpu[level]])
        return out


def _rows(manager, hier):
    """level -> for every row of the oracle's order the device's row (tests/_parity.py::MaskRecorder.replay)."""
    from oracle import sparse_ref
    to_gpu = {}
    for l in range(len(hier.coords)):
        kg = sparse_ref.pack_keys(manager.coords[l].cpu().numpy())
        ko = sparse_ref.pack_keys(hier.coords[l])
        order = np.argsort(kg)
        pos = np.searchsorted(kg[order], ko)
        assert np.array_equal(kg[order][pos], ko)
        to_gpu[l] = torch.from_numpy(order[pos])
    return to_gpu


class _Device:
    def __init__(self):
        from box2mask_amd import synth
        from box2mask_amd.config import scannet_config
        from box2mask_amd.detection_net import SelectionNet
        from oracle import sparse_ref
        self.cfg = scannet_config()
        valid, _, _, is_fg = synth.scannet_tables()
        torch.manual_seed(0)
        self.net = SelectionNet(self.cfg, 'cuda', valid, is_fg, out_channels=[96, 96, 6]).cuda()
        self.batch = R.make_batch()
        self.n_seg = self.batch['input_location'].shape[0]
        self.sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.p_cpu = {k: v.cpu() for k, v in self.sd.items()}
        self.hier = sparse_ref.Hierarchy(self.batch['vox_coords'].numpy())
        self.gws = None
        self.to_gpu = None

    def run(self, decisions):
        """One half training pass: (Pass in the oracle's row order with un-scaled gradients, launches, dtypes of the traced tensors)."""
        from box2mask_amd import _lib, nn as ME, sparse as sparse_mod
        net, batch = self.net, self.batch
        net.load_state_dict(self.sd)                 # (the running statistics moved in the pass before)
        for p in net.parameters():
            p.grad = None
        sparse_mod.REORDER_DEFAULT = False           # input row order, as the fp32 parity test
        try:
            sin = ME.SparseTensor(batch['vox_features'], batch['vox_coords'])
        finally:
            sparse_mod.REORDER_DEFAULT = True
        net.train()
        net.half_training, net._trace = True, {}
        calls, tgrad = [], {}
        _lib.set_hook(lambda name, a, meta=None: calls.append(name))
        try:
            with decisions.installed():
                out = net(sin, batch['pooling_ids'].cuda(), self.n_seg)
                if self.gws is None:
                    self.gws = R.targets({h: out[h].F.shape for h in R.HEADS})
                trace = dict(net._trace)
                for name, t in trace.items():
                    t.register_hook(lambda g, name=name: tgrad.__setitem__(name, g.detach().clone()))
                sum(((out[h].F - self.gws[h].float().cuda()) ** 2).mean() for h in R.HEADS).backward()
        finally:
            _lib.set_hook(None)
            net.half_training = False
            net._trace = None
        torch.cuda.synchronize()
        if self.to_gpu is None:
            self.to_gpu = _rows(sin.manager, self.hier)
        perm = lambda name, t: t.detach().cpu()[self.to_gpu[R.LEVEL_OF[name]]]
        dtypes = {k: v.dtype for k, v in trace.items()}
        assert all(tgrad[k].dtype == v for k, v in dtypes.items())
        p = R.Pass({h: out[h].F.detach().cpu().double() for h in R.HEADS},
                   {n: q.grad.detach().cpu().double() for n, q in net.named_parameters() if q.grad is not None},
                   {k: perm(k, v).double() for k, v in trace.items()},
                   {k: perm(k, g).double() / (R.LOSS_SCALE if dtypes[k] == torch.float16 else 1.0) for k, g in tgrad.items()})
        return p, calls, dtypes


@pytest.fixture(scope='module')
def held():
    """The device pass and the four oracle passes every test below shares."""
    d = _Device()
    assert float(d.cfg.half_loss_scale) == R.LOSS_SCALE
    with _env(ENV):
        rec = _Decisions()
        dev, calls, dtypes = d.run(rec)
    masks = rec.in_oracle_order(d.to_gpu, d.hier, d.n_seg)
    run = lambda dtype, **kw: R.oracle_pass(d.p_cpu, d.batch, d.cfg, d.hier, d.n_seg, dtype, gws=d.gws, masks=masks, **kw)
    rule = run(torch.float64)
    yard = run(torch.float32, other=rule.own)
    forced_dev = run(torch.float64, force=dev)
    forced_yard = run(torch.float64, force=yard, other=yard.own)
    h = dict(d=d, rec=rec, dev=dev, calls=calls, dtypes=dtypes, rule=rule, yard=yard, forced_dev=forced_dev, forced_yard=forced_yard)
    h['yard_whole'], h['dev_whole'] = R.whole_network(yard, rule), R.whole_network(dev, rule)
    h['yard_segments'], h['dev_segments'] = R.segments(yard, forced_yard), R.segments(dev, forced_dev)
    return h


def test_the_half_region_runs_in_binary16_and_launches_what_the_layer_table_says(held):
    assert set(held['dtypes']) == set(R.LEVEL_OF)
    for name, dt in held['dtypes'].items():
        assert dt == (torch.float16 if name in R.HALF_TRACED else torch.float32), (name, dt)
    n_conv, n_bn, n_cat = R.layer_table_counts(held['d'].p_cpu)
    st = held['rule'].storage
    assert st.count == {'to_half': 2, 'conv': n_conv, 'bn': n_bn, 'weight': n_conv}, st.count
    calls = held['calls']
    n_h = sum(1 for c in calls if c in ('b2m_conv_fwd_h', 'b2m_conv_fwd_h_stats'))
    n_apply = sum(1 for c in calls if c == 'b2m_bn_apply_h')
    n_w = sum(1 for c in calls if c == 'b2m_conv_wgrad_h')
    print('launches: b2m_conv_fwd_h* %d (storage points: %d convolutions forward, as many data gradients, %d more for the second source '
          'of an ME.cat), b2m_bn_apply_h %d (%d), b2m_conv_wgrad_h %d' % (n_h, n_conv, n_cat, n_apply, n_bn, n_w))
    assert n_h == 2 * n_conv + n_cat and n_apply == n_bn and n_w == n_conv + n_cat, (n_h, n_apply, n_w)
    assert all(bool(torch.isfinite(g).all()) for g in held['dev'].grads.values()) and len(held['dev'].grads) == 283
    print('saturation head-room (rule): largest activation %.3e, largest scaled gradient %.3e of 65504' % (st.max_activation, st.max_scaled_gradient))
    assert st.max_activation < 65504.0 and st.max_scaled_gradient < 65504.0


def test_the_whole_network_within_four_times_the_yardstick(held):
    """Heads (over the maximum and row by row), traced tensors, the 283 parameter gradients over their own maxima, the cosine."""
    R.table('whole network', held['yard_whole'], held['dev_whole'])
    bad = R.outside(held['dev_whole'], R.bounds(held['yard_whole']))
    assert not bad, ['%s: %.3e, bound %.3e' % (k, v, b) for _, k, v, b in bad[:10]]


def test_stretch_by_stretch_within_four_times_the_yardstick(held):
    """The rule forced with the device's value and gradient at every traced point: per stretch the outputs, the gradient sent back
    and the parameter gradients.  The yardstick here is 1e-6 ... 1e-3, and every deliberate mistake of
    tests/test_half_oracle_rule.py leaves these bounds."""
    b = R.segment_bounds(held['yard_segments'])
    R.table('stretch by stretch', held['yard_segments'], held['dev_segments'], b)
    assert max(v for k, v in b.items() if k.startswith('segment head/')) <= 1e-1 / 5      # a fifth of what the fp32-twin test accepts
    assert max(v for k, v in b.items() if k.startswith('segment parameter/')) <= 3e-1 / 5
    bad = R.outside(held['dev_segments'], b)
    assert not bad, ['%s: %.3e, bound %.3e' % (k, v, b_) for _, k, v, b_ in bad[:10]]


def test_relu_decisions_of_the_device_against_the_rules_own(held):
    """Where the device's decision differs from the rule's own x > 0: the fraction of a layer's elements and the largest
    |pre-activation| / rms among them, against 4 x what the yardstick's own decisions show -- from the inputs (whole network) and with
    the held pass's values in place (stretch by stretch, where a kernel that decides y > 0 wrongly cannot hide behind the forward
    distance).  Elements in (0, 2^-25] store as zero in binary16 while fmaf(x, scale, shift) > 0: counted, a negligible share."""
    for what, dev_stats, yard_stats in (('whole network', held['rule'].relu_stats, held['yard'].relu_stats),
                                        ('stretch by stretch', held['forced_dev'].relu_stats, held['forced_yard'].relu_stats)):
        yf, yw = max(s['oth_frac'] for s in yard_stats), max(s['oth_worst'] for s in yard_stats)
        df, dw = max(s['dev_frac'] for s in dev_stats), max(s['dev_worst'] for s in dev_stats)
        n = sum(s['n'] for s in dev_stats)
        tiny = sum(s['dev_tiny'] for s in dev_stats)
        print('ReLU decisions, %s: fraction yardstick %.3e | bound %.3e | device %.3e;  |pre-activation| / rms yardstick %.3e | bound %.3e | '
              'device %.3e;  stored as zero: %d of %d' % (what, yf, R.MARGIN * yf, df, yw, R.MARGIN * yw, dw, tiny, n))
        assert len(dev_stats) == len(held['rec'].masks) >= 75
        assert df <= R.MARGIN * yf and dw <= R.MARGIN * yw, (what, df, yf, dw, yw)
        assert tiny <= 1e-6 * n, (tiny, n)


# B2M_CONV_PASSTHROUGH=0: the gradient of a block input's other consumer is added by autograd behind the data-gradient kernel -- the
# sum of two binary16 tensors, rounded again -- at the 14 blocks and the 3 strided layers of the half region that pass through.  One
# more rounding of a tensor moves each element by at most 2^-11 of itself; the parameter gradients upstream are linear in these
# tensors, so 17 such tensors move one by at most 17 * 2^-11 of its scale (signs all alike, no cancellation -- an upper end, not a
# fit), and the cosine by half the square of that.
EXTRA_ROUNDINGS = 17 * 2.0 ** -11


@pytest.mark.parametrize('form', sorted(WGRAD_FORMS))
def test_the_other_forms_of_the_pass_against_the_same_rule(held, form):
    """The three forms of the weight gradient, each without the fused pass-through and without the convolution's tile statistics:
    one more device pass with the recorded decisions replayed on the device, held to the bounds of the whole-network test against
    the same rule pass."""
    d = held['d']
    env = dict(ENV, B2M_CONV_PASSTHROUGH='0', B2M_CONV_STATS_H='0', B2M_WGRAD_STREAM='0', **WGRAD_FORMS[form])
    with _env(env):
        replay = _Decisions(replay=held['rec'].masks)
        got, calls, _ = d.run(replay)
        assert replay.idx == len(replay.masks)
    assert 'b2m_conv_fwd_h_stats' not in calls and 'b2m_conv_wgrad_h' in calls
    q = R.whole_network(got, held['rule'])
    R.table('whole network, %s, no fused pass-through, no tile statistics' % form, held['yard_whole'], q, head=6)
    b = R.bounds(held['yard_whole'], {'gradient/': EXTRA_ROUNDINGS, '1 - cosine': EXTRA_ROUNDINGS ** 2 / 2})
    bad = R.outside(q, b)
    assert not bad, ['%s: %.3e, bound %.3e' % (k, v, b_) for _, k, v, b_ in bad[:10]]
