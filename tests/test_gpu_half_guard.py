"""Dynamic loss scaling for half training (box2mask_amd/half_guard.py, csrc/guard.hip) on the device:

  1. b2m_half_absmax / b2m_f32_absmax / b2m_guard_finish bit for bit against the rule of tests/_guard_rule.py at the sizes where
     the kernels take another path (no row, one row, around a wave, more than one workgroup, past the grid clamp; heads and tails of
     the 16-byte loads; padded and odd pitches; a base that is not 16-byte aligned);
  2. coverage: every half gradient tensor a training pass produces is scanned right behind the launch that produced it, and with a
     float loss scale no guard entry runs at all;
  3. a clean step in dynamic mode gives the bits of the static step; an overflowing step is skipped whole (the same sequence with the
     constant scale ruins Adam's moments); a clipped data gradient (65504, nothing non-finite) counts;
  4. two ranks: one overflows, both skip; state_dict round trip; a non-fused optimizer is refused.

"Overflow" is inf, NaN or 65504 as numbers in ordinary memory: nothing here makes a kernel fault."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _guard_rule as R

pytestmark = pytest.mark.gpu

PLANTS = (0x7bfe, 0x7bff, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x8000, 0x0001)
LARGER = 0x12345                       # a preset of *out above every binary16 magnitude: it must survive


@pytest.fixture(autouse=True)
def _no_guard_left_behind():
    from box2mask_amd import half_train as HT
    yield
    HT.guard[0] = None
    HT.loss_scale[0] = 1024.0


def _run_half(lib_call, bufs, off, ld, n, c, presets):
    """bufs: (k, L) uint16 -- k variants of one matrix; one launch each into its own word; returns the k words."""
    dev = torch.from_numpy(np.ascontiguousarray(bufs).view(np.int16)).cuda()
    out = torch.tensor(presets, dtype=torch.int64).to(torch.int32).cuda()
    for i in range(dev.shape[0]):
        lib_call('b2m_half_absmax', dev[i].data_ptr() + 2 * off, ld, n, c, out.data_ptr() + 4 * i)
    return [int(v) & 0xffffffff for v in out.tolist()]


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 1025])
def test_half_absmax_against_the_rule(n):
    from box2mask_amd import _lib
    checked = 0
    for c in (1, 7, 8, 9, 96, 100):
        for ld in (c, c + 1, c + 8):
            for off in (0, 1):
                variants, presets, want = [], [], []
                pos = R.positions(n, c) if n else {'none': None}
                base = R.half_matrix(n, c, ld, off, seed=1 + c + ld)
                zeros = R.half_matrix(n, c, ld, off, zeros=True)
                for vi, plant in enumerate(PLANTS):
                    for pi, (where, rk) in enumerate(sorted(pos.items())):
                        # (the two smallest plants go into a matrix of zeros: only there can they be the maximum)
                        buf = (zeros if plant in (0x8000, 0x0001) else base).copy()
                        if rk is not None:
                            buf[off + rk[0] * ld + rk[1]] = plant
                        preset = LARGER if (vi + pi) % 2 else (vi % 2)          # larger / smaller (0 or 1) than the answer
                        variants.append(buf); presets.append(preset)
                        want.append(R.half_absmax(buf, off, ld, n, c, preset))
                got = _run_half(_lib.call, np.stack(variants), off, ld, n, c, presets)
                assert got == want, (n, c, ld, off, [(hex(g), hex(w)) for g, w in zip(got, want) if g != w][:4])
                checked += len(want)
                if n:
                    # the padding holds 0x7fff: had it been read, every word with a small preset would be 0x7fff
                    assert all(w < R.PAD for w, p in zip(want, presets) if p != LARGER)
    assert checked == 6 * 3 * 2 * len(PLANTS) * (4 if n else 1)


@pytest.mark.parametrize('ld', [96, 104])
def test_half_absmax_past_the_grid_clamp(ld):
    """70 000 x 96: more 16-byte groups than the clamped grid has threads -- every thread strides."""
    from box2mask_amd import _lib
    n, c = 70000, 96
    base = R.half_matrix(n, c, ld, 0, seed=5)
    variants, want = [], []
    for plant, where in ((0x7bff, 'last'), (0xfc00, 'last_row_start'), (0x7e00, 'row_end'), (0x3c00, 'first')):
        buf = base.copy()
        r, k = R.positions(n, c)[where]
        buf[r * ld + k] = plant
        variants.append(buf); want.append(R.half_absmax(buf, 0, ld, n, c, 0))
    # and one in the middle, where only a striding thread gets to
    buf = base.copy()
    buf[45678 * ld + 50] = 0x7c00
    variants.append(buf); want.append(R.H_INF)
    assert _run_half(_lib.call, np.stack(variants), 0, ld, n, c, [0] * len(variants)) == want


@pytest.mark.parametrize('n', [0, 1, 3, 4, 5, 255, 256, 257, 2 ** 20 + 3])
def test_f32_absmax_against_the_rule(n):
    from box2mask_amd import _lib
    rng = np.random.default_rng(n)
    for off in (0, 1):
        base = np.full(off + n + 8, 0x7fffffff, np.uint32)                    # (around the array: a NaN above everything planted)
        base[off:off + n] = rng.integers(1, 0x3f800000, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31)
        spots = sorted({0, n - 1, n // 2, max(n - 4, 0)}) if n else [None]
        variants, presets, want = [], [], []
        for vi, plant in enumerate((0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x80000000)):
            for si, s in enumerate(spots):
                buf = base.copy()
                if plant == 0x80000000:
                    buf[off:off + n] = 0                                      # -0 among zeros: the answer is 0
                if s is not None:
                    buf[off + s] = plant
                preset = 0x7fffffff if (vi + si) % 2 else 0
                variants.append(buf); presets.append(preset)
                want.append(R.f32_absmax(buf, off, n, preset))
        dev = torch.from_numpy(np.stack(variants).view(np.int32)).cuda()
        out = torch.tensor(presets, dtype=torch.int64).to(torch.int32).cuda()
        for i in range(dev.shape[0]):
            _lib.call('b2m_f32_absmax', dev[i].data_ptr() + 4 * off, n, out.data_ptr() + 4 * i)
        got = [int(v) & 0xffffffff for v in out.tolist()]
        assert got == want, (n, off, [(hex(g), hex(w)) for g, w in zip(got, want) if g != w][:4])


def test_guard_finish_truth_table():
    from box2mask_amd import _lib
    steps = skipped = 0
    counters = torch.zeros(2, dtype=torch.int32, device='cuda')
    for h in (0, R.H_MAXF - 1, R.H_MAXF, R.H_INF, R.H_NAN):
        for f in (0, R.F_INF - 1, R.F_INF, R.F_NAN):
            flags = torch.tensor([h, f], dtype=torch.int32, device='cuda')
            found = torch.full((), 0.5, device='cuda')
            _lib.call('b2m_guard_finish', flags.data_ptr(), found.data_ptr(), counters.data_ptr())
            want, (steps, skipped) = R.finish((h, f), (steps, skipped))
            assert found.item() == want and found.item() in (0.0, 1.0), (hex(h), hex(f))
            assert counters.tolist() == [steps, skipped]
            assert flags.tolist() == [h, f]                                   # (left as they were)
    assert steps == 20 and skipped == 20 - 2 * 2


# ---------------------------------------------------------------- the passes
def _dyn_net():
    from test_gpu_half_train import _net_and_batch
    from box2mask_amd.half_guard import HalfScaler
    net, batch, cfg = _net_and_batch()
    return net, batch, cfg, HalfScaler


def test_every_half_gradient_of_a_pass_is_scanned(monkeypatch):
    """One training pass of the small scene of tests/test_gpu_half_train.py with the call observer: in backward, every b2m_conv_fwd_h
    launch (a data gradient) and both outputs of every b2m_bn_bwd_apply_h are followed at once by a b2m_half_absmax of the same
    pointer, rows, columns and pitch; with a float loss scale the same pass calls no guard entry (and is otherwise the same list)."""
    from box2mask_amd import _lib, nn as ME
    net, batch, cfg, HalfScaler = _dyn_net()
    S_ = batch['input_location'].shape[0]

    def run(scale):
        cfg.half_loss_scale = scale
        net.half_training = True
        for p in net.parameters():
            p.grad = None
        calls, mark = [], [None]
        _lib.set_hook(lambda name, a, meta=None: calls.append((name, a)))
        try:
            out = net(ME.SparseTensor(batch['vox_features'], batch['vox_coords']), batch['pooling_ids'].cuda(), S_)
            loss = sum((out[h].F ** 2).mean() for h in ('mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'))
            mark[0] = len(calls)
            loss.backward()
        finally:
            _lib.set_hook(None)
            net.half_training = False
        torch.cuda.synchronize()
        return calls, mark[0]
    net._half_scaler = HalfScaler()
    run(1024.0)                      # (the first pass of a process packs every half weight image on first use: not the list to compare)
    dyn, b0 = run('dynamic')
    guard_names = ('b2m_half_absmax', 'b2m_f32_absmax', 'b2m_guard_finish')
    assert not any(n in guard_names for n, _ in dyn[:b0])                      # the forward pass has nothing to scan
    n_conv = n_bn = 0
    for i in range(b0, len(dyn)):
        name, a = dyn[i]
        if name == 'b2m_conv_fwd_h':
            n_conv += 1
            expect = [(a[13], a[14], a[12], a[15])]                            # (pointer, pitch, rows, columns) of the result
        elif name == 'b2m_bn_bwd_apply_h':
            n_bn += 1
            expect = [(a[17], a[18], a[6], a[7])] + ([(a[19], a[20], a[6], a[7])] if a[19] is not None else [])
        else:
            continue
        for k, e in enumerate(expect):
            nm, b = dyn[i + 1 + k]
            assert nm == 'b2m_half_absmax' and (b[0], b[1], b[2], b[3]) == e, (i, name, nm)
    assert n_conv >= 36 and n_bn >= 36, (n_conv, n_bn)
    n_scan = sum(1 for n, _ in dyn if n == 'b2m_half_absmax')
    print('dynamic: %d half scans per pass behind %d data-gradient launches and %d BatchNorm backward launches' % (n_scan, n_conv, n_bn))
    assert int(net._half_scaler.flags[0]) > 0                                  # something was seen
    # the constant scale: no guard entry, and the launch list is the dynamic one without its scans
    static, _ = run(1024.0)
    assert not any(n in guard_names for n, _ in static)
    assert [n for n, _ in static] == [n for n, _ in dyn if n not in guard_names]


def _model(scale, interval=2000, seed=7, **kw):
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    torch.manual_seed(seed)
    model = Model(scannet_config(half_training=True, half_loss_scale=scale, half_growth_interval=interval, **kw), *synth.scannet_tables())
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    if hasattr(model, 'attach_optimizer'):
        model.attach_optimizer(opt)
    return model, opt


@pytest.fixture(scope='module')
def small_batch():
    from box2mask_amd import synth
    return synth.make_batch(8, seed0=60, target_voxels=6000, pts_per_m2=6000.0)


def _step(model, opt, batch, factor=1.0):
    opt.zero_grad()
    losses, pred = model.compute_loss_detection(batch, 150)
    (losses['optimization_loss'] * factor).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.detection_model.named_parameters() if p.grad is not None}
    opt.step()
    return {k: v.detach().clone() for k, v in pred.items()}, grads


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_clean_step_gives_the_bits_of_the_static_step(monkeypatch):
    """Dynamic (from 1024) against the constant 1024 on the same weights and batch, bit for bit: heads, all 283 parameter
    gradients, the weights after one fused Adam step.

    The batch.  Two runs of the CONSTANT-scale step already differ where they can: b2m_conv_wgrad_h adds the partial blocks of its
    tile chunks into dW with fp32 atomics and has no ordered form (include/b2m.h; B2M_DETERMINISTIC=1 orders everything else).  On
    8 x 6000 voxels static against static differs in 40 of the 283 gradients (the convolutions of the half region, 3e-7 of their
    maximum), and dynamic against static by the same 40 -- which says nothing about the guard.  With at most 64 tiles (4096 rows)
    at stride 1 and chunks of 64 tiles (B2M_WGRAD_MIN_TILES=64) every map of the half region is ONE chunk: every element of dW has
    one adder, the sum has one order, and equal bits can be asked for (measured: static against static 0 of 283 differ).

    The loss.  On so few rows the mean loss's gradient per row is large: at scale 1024 this batch OVERFLOWS (largest half gradient
    3.2e5 -- the guard skips the step, the constant scale writes 14 non-finite weight gradients).  A clean step is what this test
    is about, so both modes take the loss times 2^-8 (exact): largest half gradient 1245, everything finite."""
    from box2mask_amd import half_train as HT, synth, _lib
    monkeypatch.setenv('B2M_DETERMINISTIC', '1')
    monkeypatch.setenv('B2M_WGRAD_MIN_TILES', '64')
    _lib.reload_env()
    small_batch = synth.make_batch(8, seed0=60, target_voxels=150, pts_per_m2=6000.0)
    assert small_batch['vox_coords'].shape[0] <= 64 * 64
    res = {}
    for mode in ('dynamic', 1024.0):
        model, opt = _model(mode, interval=2)
        factor = 2.0 ** -8
        pred, grads = _step(model, opt, small_batch, factor)
        res[mode] = (pred, grads, {n: p.detach().clone() for n, p in model.detection_model.named_parameters()})
        if mode == 'dynamic':
            torch.cuda.synchronize()
            assert model.half_scaler.found_inf.item() == 0.0
            assert HT.loss_scale[0] == 1024.0
            _step(model, opt, small_batch, factor)
            assert HT.loss_scale[0] == 1024.0                  # one clean step: the tracker stands at 1
            _step(model, opt, small_batch, factor)
            assert HT.loss_scale[0] == 2048.0                  # two clean steps at interval 2: the third pass runs at 2048
            st = model.half_scaler.stats()
            assert st['steps'] == 3 and st['skipped'] == 0 and 0.0 < st['max_half_grad'] < 65504.0
    (pd, gd, wd), (ps, gs, ws) = res['dynamic'], res[1024.0]
    assert set(pd) == set(ps) and all(_same(pd[h], ps[h]) for h in ps)
    assert set(gd) == set(gs) and len(gs) == 283
    monkeypatch.undo()
    _lib.reload_env()
    differ = [n for n in gs if not _same(gd[n], gs[n])]
    print('dynamic against static: %d of %d gradients differ %s' % (len(differ), len(gs), differ[:3]))
    assert all(bool(torch.isfinite(g).all()) for g in gs.values())
    assert differ == []
    assert [n for n in ws if not _same(wd[n], ws[n])] == []


def _opt_state(opt):
    out = {}
    for i, p in enumerate(p for g in opt.param_groups for p in g['params']):
        st = opt.state.get(p, {})
        out[i] = (p.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone(), st['step'].clone())
    return out


def test_overflowing_step_is_skipped_whole(monkeypatch, small_batch):
    """A loss a million times too large: at scale 1024 the gradient entering the half region is inf.  Dynamic: found, nothing of
    the optimizer's state moves, the next pass runs at 512, a clean step follows.  The constant scale: the same sequence leaves
    non-finite moments behind -- what the guard is for."""
    from box2mask_amd import half_train as HT
    monkeypatch.setenv('B2M_DETERMINISTIC', '1')
    model, opt = _model('dynamic')
    _step(model, opt, small_batch)                              # (a clean step first: the moments exist)
    before = _opt_state(opt)
    _step(model, opt, small_batch, factor=1e6)
    torch.cuda.synchronize()
    assert model.half_scaler.found_inf.item() == 1.0
    after = _opt_state(opt)
    assert len(before) == 283
    for i in before:
        assert all(_same(a, b) for a, b in zip(before[i], after[i])), i
    _step(model, opt, small_batch)
    assert HT.loss_scale[0] == 512.0
    st = model.half_scaler.stats()
    assert st['skipped'] == 1 and st['steps'] == 3 and st['scale'] == 512.0
    assert model.half_scaler.found_inf.item() == 0.0
    final = _opt_state(opt)
    moved = sum(1 for i in before if not _same(before[i][0], final[i][0]))
    assert moved > 250, moved
    assert all(bool(torch.isfinite(t).all()) for i in final for t in final[i])
    assert all(float(final[i][3]) == 2.0 for i in final)       # two steps taken, one skipped
    # the same three steps at the constant 1024
    model, opt = _model(1024.0)
    assert model.half_scaler is None
    _step(model, opt, small_batch)
    _step(model, opt, small_batch, factor=1e6)
    _step(model, opt, small_batch)
    final = _opt_state(opt)
    bad = sum(1 for i in final if not (torch.isfinite(final[i][1]).all() and torch.isfinite(final[i][2]).all()))
    print('constant scale: %d of %d parameters end with non-finite moments' % (bad, len(final)))
    assert bad > 0


@pytest.fixture(scope='module')
def maps():
    from test_gpu_ops import _scene
    from box2mask_amd.sparse import CoordinateManager
    m = CoordinateManager(_scene()['vox_coords'])
    m.ensure_level(2)
    return m


def test_clipped_data_gradient_counts_as_found(maps):
    """The data-gradient launch clamps: dy = 2048 through a centre tap of 64 would be 131072 and is stored as 65504 -- nothing
    anywhere is non-finite, the flag word reads exactly 0x7bff, and the step counts as found."""
    from box2mask_amd import half_train as HT, _lib
    from box2mask_amd.half_guard import HalfScaler
    sc = HalfScaler(init_scale=1.0)
    HT.guard[0] = sc
    rb = maps.rulebook_same(0, 3)
    n, c = maps.n(0), 32
    x = torch.randn(n, c, device='cuda').half().requires_grad_(True)
    w = torch.zeros(27, c, c, device='cuda')
    w[13] = 64.0 * torch.eye(c, device='cuda')
    w.requires_grad_(True)
    y = HT.conv(x, None, w, rb, rb, True, n)
    y.backward(torch.full((n, c), 2048.0, device='cuda').half())
    torch.cuda.synchronize()
    assert HT.loss_scale[0] == 1.0
    assert bool(torch.isfinite(x.grad.float()).all()) and float(x.grad.float().abs().max()) == 65504.0
    assert bool(torch.isfinite(w.grad).all())
    assert sc.flags.tolist() == [R.H_MAXF, 0]
    _lib.call('b2m_guard_finish', sc.flags.data_ptr(), sc.found_inf.data_ptr(), sc.counters.data_ptr())
    assert sc.found_inf.item() == 1.0 and sc.counters.tolist() == [1, 1]


def test_batchnorm_gradient_that_overflows_reads_inf():
    from box2mask_amd import half_train as HT
    from box2mask_amd.half_guard import HalfScaler
    sc = HalfScaler(init_scale=1.0)
    HT.guard[0] = sc
    n, c = 3000, 96
    torch.manual_seed(3)
    x = (torch.randn(n, c, device='cuda') * 1.5 + 0.3).half().requires_grad_(True)
    gamma = torch.full((c,), 64.0, device='cuda', requires_grad=True)
    beta = torch.zeros(c, device='cuda', requires_grad=True)
    y = HT.batch_norm(x, gamma, beta, torch.zeros(c, device='cuda'), torch.ones(c, device='cuda'), 0.1, 1e-5, None, False)
    gy = (torch.randn(n, c, device='cuda') * 2000.0).half()
    assert bool(torch.isfinite(gy.float()).all())
    y.backward(gy)
    torch.cuda.synchronize()
    g = x.grad.float()
    assert bool(torch.isinf(g).any()) and not bool(torch.isnan(g).any())
    assert sc.flags.tolist() == [R.H_INF, 0]


def test_state_dict_round_trip(small_batch):
    model, opt = _model('dynamic', interval=2)
    _step(model, opt, small_batch)
    _step(model, opt, small_batch, factor=1e6)
    _step(model, opt, small_batch)
    sd = model.half_scaler.state_dict()
    assert sd == {'scale': 512.0, 'growth_tracker': 1, 'steps': 3, 'skipped': 1}
    assert not any('scale' in k or 'guard' in k for k in model.state_dict())   # (Model.state_dict's keys are the reference's)
    from box2mask_amd.half_guard import HalfScaler
    other = HalfScaler(growth_interval=2)
    other.load_state_dict(sd)
    assert other.state_dict() == sd and other.counters.tolist() == [3, 1]
    assert other.scale == 512.0 and other.growth_tracker == 1
    with pytest.raises(ValueError):
        other.load_state_dict(dict(sd, scale=1000.0))


def test_attach_refuses_an_optimizer_that_is_not_fused():
    model, _ = _model('dynamic')
    with pytest.raises(TypeError, match='fused'):
        model.attach_optimizer(torch.optim.Adam(model.parameters(), lr=1e-3))
    with pytest.raises(TypeError, match='fused'):
        model.half_scaler.attach(torch.optim.SGD(model.parameters(), lr=1e-3))


# ---------------------------------------------------------------- two ranks on one GPU
def _rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      B2M_DETERMINISTIC='1')
    import torch.distributed as dist
    from box2mask_amd import synth, half_train as HT
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    from box2mask_amd.parallel import init_distributed, shard_scenes
    torch.cuda.set_device(0)
    init_distributed('gloo')
    torch.manual_seed(0)
    cfg = scannet_config(multigpu=True, half_training=True, half_loss_scale='dynamic')
    model = Model(cfg, *synth.scannet_tables(), device='cuda:0')
    batch = synth.collate([synth.make_scene(100 + s, target_voxels=2000, pts_per_m2=6000.0) for s in shard_scenes(8, rank, world)])
    model.train()
    opt = model.attach_optimizer(torch.optim.Adam(model.parameters(), lr=1e-3, fused=True))
    sample = lambda: torch.cat([p.detach().reshape(-1)[:64] for p in model.parameters()]).cpu().numpy()

    def step(factor):
        opt.zero_grad()
        (model.compute_loss(batch, 150)['optimization_loss'] * factor).backward()
        scale = HT.loss_scale[0]
        opt.step()
        torch.cuda.synchronize()
        return scale, float(model.half_scaler.found_inf.item())
    w0 = sample()
    s1, f1 = step(1e6 if rank == 1 else 1.0)                   # only rank 1 overflows
    w1 = sample()
    s2, f2 = step(1.0)
    w2 = sample()
    q.put((rank, {'scales': (s1, s2), 'found': (f1, f2), 'w0': w0, 'w1': w1, 'w2': w2, 'stats': model.half_scaler.stats()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_one_rank_overflows_both_ranks_skip():
    """Two gloo ranks on this one GPU (spawned before this process has touched it for them: the pattern of tests/test_gpu_dp.py).
    Only rank 1's loss is too large; the flag words are MAX-all-reduced, so both ranks skip the step, keep identical weights and
    run the next pass at 512."""
    from test_gpu_dp import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=500) for _ in range(2))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in (0, 1):
        assert res[r]['found'] == (1.0, 0.0), (r, res[r]['found'])
        assert res[r]['scales'] == (1024.0, 512.0), (r, res[r]['scales'])
        assert np.array_equal(res[r]['w0'], res[r]['w1'])                      # skipped: nothing moved
        assert not np.array_equal(res[r]['w1'], res[r]['w2']) and np.all(np.isfinite(res[r]['w2']))
        assert res[r]['stats']['skipped'] == 1 and res[r]['stats']['steps'] == 2
    for k in ('w0', 'w1', 'w2'):
        assert np.array_equal(res[0][k], res[1][k]), k
