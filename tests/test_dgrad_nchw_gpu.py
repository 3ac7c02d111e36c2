"""conv3's data gradient reading FC1's gradient in NCHW (rth_conv_dgrad_relu_nchw_prepacked, r15:
conv3's own ReLU mask and the channels-last masked gradient in the launch that already masks for
conv2, conv3's bias slabs from a small launch in the old order) against the two launches it
replaces, rth_relu_bias_grad_nchw + rth_conv_dgrad_relu_prepacked, of the same library; and the
learner with the switch on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CONV1, CONV2, CONV3 = (4, 84, 84, 32, 8, 4), (32, 20, 20, 64, 4, 2), (64, 9, 9, 64, 3, 1)


def _shape(inp, cin, h, w, cout, k, s):
    from reth_amd import _lib

    return _lib.ConvShape(inp, cin, h, w, cout, k, k, s)


def _within_sum_bound(got, terms):
    """|got - fp64 sum| <= 1e-6 * sum |terms| + 1e-12 per channel; terms [rows, C]"""
    t = terms.double().cpu()
    exact, scale = t.sum(0), t.abs().sum(0)
    return bool(((got.double().cpu() - exact).abs() <= 1e-6 * scale + 1e-12).all())


# n: 1 = one workgroup with one sample; 5 = the one-sample form over several workgroups; 301 = an
# odd count under the two-sample instantiation (151 workgroups on 256 CUs: the last one partial);
# 512 = the learner's shape, 256 slabs
@pytest.mark.parametrize("n", [1, 5, 301, 512])
def test_conv_dgrad_relu_nchw_prepacked(dev, n):
    from reth_amd import _lib

    byref, st = _lib.ctypes.byref, _lib.stream_ptr()
    cin, h, wd, cout, k, s = CONV3
    ho, P = h - k + 1, (h - k + 1) ** 2
    shape = _shape(_lib.CONV_F32_NHWC, *CONV3)
    assert _lib.lib().rth_conv_dgrad_relu_nchw_supported(byref(shape)) == 1
    gen = torch.Generator(device=dev).manual_seed(1500 + n)
    g = torch.randn((n, cout, ho, ho), device=dev, generator=gen)  # NCHW, as FC1 leaves it
    y3 = torch.relu(torch.randn((n, cout, ho, ho), device=dev, generator=gen))
    flat = y3.view(-1)  # the strict > 0: -0.0 and a subnormal among the positives
    pos = torch.nonzero(flat > 0).view(-1)
    flat[pos[0:40:4]] = -0.0
    flat[pos[1:40:4]] = 1e-40
    w = (torch.randn((cout, cin, k, k), device=dev, generator=gen) * 0.05).contiguous(memory_format=torch.channels_last)
    y2 = torch.relu(torch.randn((n, cin, h, wd), device=dev, generator=gen)).contiguous(
        memory_format=torch.channels_last)
    assert int((y2 == 0).sum()) > 0
    work = torch.empty(_lib.lib().rth_conv_dgrad_workspace(byref(shape)) // 4, device=dev)
    scratch = torch.empty((n, cin, h, wd), device=dev).contiguous(memory_format=torch.channels_last)
    gy_any = torch.zeros((n, cout, ho, ho), device=dev).contiguous(memory_format=torch.channels_last)
    _lib.call("rth_conv_dgrad_ws", byref(shape), gy_any.data_ptr(), n, w.data_ptr(), scratch.data_ptr(),
              work.data_ptr(), st)  # packs the flipped kernel into work, as the learner's pack launch

    def bias_ws():
        return torch.empty(_lib.lib().rth_relu_bias_grad_workspace(64), dtype=torch.uint8, device=dev)

    # conv1's reduce launch finishes the deferred jobs (a small conv1 problem beside them)
    c1 = _shape(_lib.CONV_U8_CHW, *CONV1)
    stk = torch.randint(0, 256, (3, 4, 84, 84), dtype=torch.uint8, device=dev, generator=gen)
    gc = torch.randn((3, 20, 20, 32), device=dev, generator=gen)
    yc = torch.randn((3, 20, 20, 32), device=dev, generator=gen)
    wsc = torch.empty(_lib.lib().rth_conv_wgrad_workspace(byref(c1)), dtype=torch.uint8, device=dev)

    def finish(jobs):
        arr = (_lib.BiasDeferred * len(jobs))(*jobs)
        gw, gb = torch.empty((32, 8, 8, 4), device=dev), torch.empty(32, device=dev)
        _lib.call("rth_conv_relu_wgrad_ex", byref(c1), stk.data_ptr(), None, 3, gc.data_ptr(), yc.data_ptr(),
                  gw.data_ptr(), gb.data_ptr(), wsc.data_ptr(), arr, len(jobs), None, 0, st)

    def nan(*shp):
        return torch.full(shp, float("nan"), device=dev)

    # the two launches of the same library
    gy_ref = nan(n, cout, ho, ho).contiguous(memory_format=torch.channels_last)
    gx_ref = nan(n, cin, h, wd).contiguous(memory_format=torch.channels_last)
    db3_ref, db2_ref, ws3, ws2 = nan(cout), nan(cin), bias_ws(), bias_ws()
    _lib.call("rth_relu_bias_grad_nchw", g.data_ptr(), y3.data_ptr(), gy_ref.data_ptr(), None, ws3.data_ptr(), n,
              cout, P, st)  # (no db: the slabs wait for the deferred job, as in the learner)
    slabs = _lib.ctypes.c_int64(-1)
    _lib.call("rth_conv_dgrad_relu_prepacked", byref(shape), gy_ref.data_ptr(), n, work.data_ptr(), y2.data_ptr(),
              gx_ref.data_ptr(), ws2.data_ptr(), byref(slabs), st)
    finish([_lib.BiasDeferred(ws3.data_ptr(), db3_ref.data_ptr(), n * P, cout, 0),
            _lib.BiasDeferred(ws2.data_ptr(), db2_ref.data_ptr(), n * h * wd, cin, slabs.value)])
    torch.cuda.synchronize()

    dbs = []
    for _ in range(2):
        gy = nan(n, cout, ho, ho).contiguous(memory_format=torch.channels_last)
        gx = nan(n, cin, h, wd).contiguous(memory_format=torch.channels_last)
        db3, db2, ws3, ws2 = nan(cout), nan(cin), bias_ws(), bias_ws()
        slabs = _lib.ctypes.c_int64(-1)
        _lib.call("rth_conv_dgrad_relu_nchw_prepacked", byref(shape), g.data_ptr(), y3.data_ptr(), n, work.data_ptr(),
                  y2.data_ptr(), gy.data_ptr(), gx.data_ptr(), ws3.data_ptr(), ws2.data_ptr(), byref(slabs), st)
        assert 1 <= slabs.value <= n
        if n > 256:
            assert slabs.value < n, "a multi-sample instantiation is what this n is here for"
        finish([_lib.BiasDeferred(ws3.data_ptr(), db3.data_ptr(), n * P, cout, 0),
                _lib.BiasDeferred(ws2.data_ptr(), db2.data_ptr(), n * h * wd, cin, slabs.value)])
        torch.cuda.synchronize()
        assert torch.equal(gy, gy_ref)
        assert torch.equal(gx, gx_ref)
        dbs.append((db3.clone(), db2.clone()))
    assert torch.equal(dbs[0][0], dbs[1][0]) and torch.equal(dbs[0][1], dbs[1][1])
    t3 = gy_ref.permute(0, 2, 3, 1).reshape(-1, cout)
    t2 = gx_ref.permute(0, 2, 3, 1).reshape(-1, cin)
    assert _within_sum_bound(dbs[0][0], t3) and _within_sum_bound(db3_ref, t3)
    assert _within_sum_bound(dbs[0][1], t2) and _within_sum_bound(db2_ref, t2)
    # both bias gradients keep the two-launch path's bits: conv2's slabs are the existing epilogue's,
    # conv3's are summed in rth_relu_bias_grad_nchw's order
    assert torch.equal(dbs[0][0], db3_ref) and torch.equal(dbs[0][1], db2_ref)

    conv2 = _shape(_lib.CONV_F32_NHWC, *CONV2)
    assert _lib.lib().rth_conv_dgrad_relu_nchw_supported(byref(conv2)) == 0
    with pytest.raises(_lib.RethHipError, match="only conv3"):
        _lib.call("rth_conv_dgrad_relu_nchw_prepacked", byref(conv2), g.data_ptr(), y3.data_ptr(), n, work.data_ptr(),
                  y2.data_ptr(), gy.data_ptr(), gx.data_ptr(), ws3.data_ptr(), ws2.data_ptr(), byref(slabs), st)


def test_learner_dgrad_nchw_on_off(dev, monkeypatch):
    """the learner's gradients on B = 6 uint8 stacks with DGRAD_NCHW on and off: every gradient
    bit-identical, conv3's bias gradient included (and within the summation bound of the fp64 sum
    of the masked gradient); the off arm issues rth_relu_bias_grad_nchw, the on arm does not"""
    from reth_amd import fused_learner
    from reth_amd.solver import Box, DQNSolver, Discrete

    B = 6
    gen = torch.Generator(device=dev).manual_seed(15)
    frames = torch.randint(0, 256, (2 * B, 4, 84, 84), dtype=torch.uint8, device=dev, generator=gen)
    batch = [frames[:B], torch.randint(0, 6, (B,), device=dev, generator=gen),
             (torch.rand(B, device=dev, generator=gen) < 0.3).float(), frames[B:],
             (torch.rand(B, device=dev, generator=gen) < 0.1).float()]
    isw = torch.rand(B, device=dev, generator=gen, dtype=torch.float64) + 0.5
    torch.manual_seed(15)
    solver = DQNSolver(Box(0, 255, (4, 84, 84)), Discrete(6), gamma=0.99, clip_value=40, double_q=True, dueling=True,
                       learning_rate=1e-4, adam_epsilon=1.5e-4, update_target_interval=100, device=dev, n_step=3,
                       channels_last=True)
    assert fused_learner.eligible(solver.q_network, batch[0], batch[3])
    seen = {}  # device pointer -> tensor, of everything the pass hands to the library
    real_ptr, real_call = fused_learner.ptr, fused_learner.call

    def spy_ptr(t):
        if t is not None:
            seen[t.data_ptr()] = t
        return real_ptr(t)

    monkeypatch.setattr(fused_learner, "ptr", spy_ptr)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(fused_learner, "DGRAD_NCHW", on)
        names, masked = [], []

        def spy_call(name, *args):
            names.append(name)
            rc = real_call(name, *args)
            if name == "rth_relu_bias_grad_nchw":
                masked.append(seen[args[2]].clone())
            if name == "rth_conv_dgrad_relu_nchw_prepacked":
                masked.append(seen[args[6]].clone())
            return rc

        monkeypatch.setattr(fused_learner, "call", spy_call)
        solver.compute_grads(batch, weights=isw)
        torch.cuda.synchronize()
        assert ("rth_relu_bias_grad_nchw" in names) == (not on)
        assert ("rth_conv_dgrad_relu_nchw_prepacked" in names) == on
        assert len(masked) == 1
        res[on] = ({k: p.grad.clone() for k, p in solver.q_network.named_parameters()}, masked[0])
    assert torch.equal(res[True][1], res[False][1])
    conv3_bias = solver.q_network._convs()[2].bias
    name3 = [k for k, p in solver.q_network.named_parameters() if p is conv3_bias]
    assert len(name3) == 1
    terms = res[False][1].permute(0, 2, 3, 1).reshape(-1, 64)
    for k in res[True][0]:
        if k == name3[0]:
            assert _within_sum_bound(res[True][0][k], terms) and _within_sum_bound(res[False][0][k], terms)
        assert torch.equal(res[True][0][k], res[False][0][k]), k
