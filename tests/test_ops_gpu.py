"""GPU parity of every C-ABI kernel against plain fp32 torch CPU ops of the same reference op (tolerances
stated per test; integer/index results bit-exact).  Calls go through the C ABI via seghiero_amd.ops."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from seghiero_amd import ops as o
    return o


DEV = "cuda:0"


def nhwc(t):
    """CPU NCHW tensor -> GPU logical-NCHW tensor with NHWC memory."""
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def wl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def close(a, b, rtol, atol, msg=""):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


CONV_CASES = [
    # n, h, w, cin, cout, k, stride, pad, dil
    (2, 16, 16, 64, 64, 1, 1, 0, 1),
    (2, 16, 16, 64, 256, 1, 1, 0, 1),
    (2, 17, 13, 32, 48, 3, 1, 1, 1),
    (2, 16, 16, 128, 128, 3, 2, 1, 1),
    (2, 15, 15, 64, 128, 1, 2, 0, 1),
    (1, 32, 32, 4, 64, 7, 2, 3, 1),       # stem (Cin padded 3->4)
    (2, 8, 8, 560, 512, 1, 1, 0, 1),      # K tail: 560 = 17.5 * 32
    (3, 9, 7, 16, 13, 1, 1, 0, 1),        # Cout not a multiple of 4 (cls_seg)
    (2, 12, 12, 32, 32, 3, 1, 12, 12),    # dilated dense conv
    (16, 1, 1, 64, 32, 1, 1, 0, 1),       # image-pool conv: M = batch
    (2, 40, 40, 64, 160, 3, 1, 1, 1),
    (2, 17, 13, 32, 64, 3, 2, 1, 1),      # stride-2 3x3 on odd sizes (parity-class dgrad)
    (1, 9, 9, 64, 32, 5, 2, 2, 1),        # stride-2 5x5
    (2, 12, 12, 256, 64, 3, 1, 1, 1),     # long K, few tiles: split-K fprop (4 slices) + reduce with bias / BN statistics
    (2, 12, 12, 64, 256, 3, 1, 1, 1),     # ... and split-K dgrad (+ addend), M = 288 not a multiple of 64
    (2, 2, 3, 512, 512, 3, 1, 1, 1),      # layer4 at a tiny input: M = 12, K = 4608 -> 8 K slices
    # M large enough (>= 512 blocks) for the 1024-thread 256x256 tiles and the 768-thread 256x192 ones (N = 272: 384 vs 512 columns)
    (1, 370, 370, 64, 256, 1, 1, 0, 1),
    (1, 370, 370, 256, 64, 1, 1, 0, 1),
    (1, 370, 370, 272, 272, 1, 1, 0, 1),
    (1, 372, 372, 32, 272, 3, 1, 1, 1),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fprop_dgrad_wgrad(ops, case):
    n, h, w, cin, cout, k, s, p, d = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g)
    ref = F.conv2d(x, wt, bias, s, p, d)
    ho, wo = ref.shape[2:]
    xg, wg = nhwc(x), wl(wt)
    ldy = ops.pad4(cout)
    y = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    part = ops.conv_partials(n * ho * wo, cout, DEV)
    ops.conv_fprop(xg, wg, bias.to(DEV), y, None, s, p, d)
    close(y, ref, 2e-5, 2e-5, "fprop+bias")
    y2 = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    ops.conv_fprop(xg, wg, None, y2, part, s, p, d)
    ref_nb = F.conv2d(x, wt, None, s, p, d)
    close(y2, ref_nb, 2e-5, 2e-5, "fprop")
    # BN statistics from the epilogue's centred (sum, M2) partials
    coefs = ops.bn_finalize(part, n * ho * wo, None, None, 1e-5, 0.1, None, None, cout, DEV, rows=64)
    close(coefs[0], ref_nb.mean((0, 2, 3)), 1e-4, 1e-5, "stat mean")
    close(coefs[1], 1.0 / torch.sqrt(ref_nb.var((0, 2, 3), unbiased=False) + 1e-5), 1e-4, 1e-5, "stat invstd")
    # backward
    dy = torch.randn(ref.shape, generator=g)
    xr = x.clone().requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, s, p, d).backward(dy)
    dyg = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    dyg.copy_(dy.to(DEV))
    dx = ops.new_act(n, cin, h, w, DEV)
    ops.conv_dgrad(dyg, wg, dx, s, p, d)
    close(dx, xr.grad, 1e-4, 1e-4, "dgrad")
    add = torch.randn(x.shape, generator=g)
    dx2 = ops.new_act(n, cin, h, w, DEV)
    ops.conv_dgrad(dyg, wg, dx2, s, p, d, addend=nhwc(add))
    close(dx2, xr.grad + add, 1e-4, 1e-4, "dgrad+addend")
    if k == 1 and p == 0:
        dx3 = nhwc(add.clone())
        ops.conv_dgrad(dyg, wg, dx3, s, p, d, mode=1)
        close(dx3, xr.grad + add, 1e-4, 1e-4, "dgrad scatter/accumulate")
    dw = torch.empty_like(wg)
    ops.conv_wgrad(xg, dyg, dw, s, p, d)
    close(dw, wr.grad, 2e-4, 2e-4 * float(wr.grad.abs().max()), "wgrad")


FUSED_CASES = [
    # n, h, w, cin, cout, k, pad, dil
    (2, 16, 16, 64, 64, 1, 0, 1),
    (2, 20, 18, 64, 256, 1, 0, 1),
    (2, 17, 19, 32, 48, 3, 1, 1),         # zero padding must stay zero AFTER the activation; N <= 64 tile
    (2, 16, 16, 128, 128, 3, 1, 1),
    (2, 16, 16, 560, 512, 1, 0, 1),       # K = 560: last half-tile masked
    (2, 12, 16, 256, 64, 3, 1, 1),        # split-K fprop with the fused loader
    (2, 16, 16, 128, 256, 3, 1, 1),       # split-K dgrad (K = 2304, 8 tiles): BatchNorm-backward front half in the slab reduce
    (1, 160, 160, 64, 128, 1, 0, 1),      # many tiles
    (2, 16, 16, 32, 32, 3, 6, 6),         # dilated
]


@pytest.mark.parametrize("case", FUSED_CASES)
def test_conv_fused_batchnorm_hooks(ops, case):
    """The three fused forms of conv -> BN -> ReLU -> conv chains (resnet.py:65-73, sep_aspp_contrast_head.py:56-61) against torch:
    fprop / wgrad reading their input through relu(x*scale+shift) in the loader, and dgrad emitting g = relumask * dx plus the
    (sum g, sum g*xhat) partials of the producer's BatchNorm backward from its epilogue."""
    n, h, w, cin, cout, k, p, d = case
    g = torch.Generator().manual_seed(sum(case))
    raw = torch.randn(n, cin, h, w, generator=g)                       # raw output of the producer conv
    scale = torch.randn(cin, generator=g)                               # both signs
    shift = 0.3 * torch.randn(cin, generator=g)
    mean = 0.2 * torch.randn(cin, generator=g)
    invstd = 0.5 + torch.rand(cin, generator=g)
    coefs = torch.stack([mean, invstd, scale, shift]).to(DEV).contiguous()
    act = torch.relu(raw * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    ar = act.clone().requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    ref = F.conv2d(ar, wr, None, 1, p, d)
    ho, wo = ref.shape[2:]
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    rawg, wg = nhwc(raw), wl(wt)
    ldy = ops.pad4(cout)
    # ---- fprop through the loader + BN statistics of ITS output
    y = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    part = ops.conv_partials(n * ho * wo, cout, DEV)
    assert ops.conv_fprop_aff(rawg, coefs, wg, None, y, part, 1, p, d)
    close(y, ref, 2e-5, 2e-5, "fprop through BN+ReLU")
    st = ops.bn_finalize(part, n * ho * wo, None, None, 1e-5, 0.1, None, None, cout, DEV, rows=64)
    close(st[0], ref.detach().mean((0, 2, 3)), 1e-4, 1e-5, "stat mean")
    # ---- wgrad through the loader
    dyg = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    dyg.copy_(dy.to(DEV))
    if ops.wgrad_aff_ok(rawg, wg, 1, p, d):
        dw = torch.empty_like(wg)
        ops.conv_wgrad(rawg, dyg, dw, 1, p, d, aff=coefs)
        close(dw, wr.grad, 2e-4, 2e-4 * float(wr.grad.abs().max()), "wgrad through BN+ReLU")
    # ---- dgrad with the BatchNorm-backward front half in the epilogue (with and without an addend)
    for add in (None, torch.randn(raw.shape, generator=g)):
        gbuf = ops.new_act(n, cin, h, w, DEV)
        bpart = torch.empty((-(-n * h * w // 64), 2, cin), device=DEV)
        assert ops.conv_dgrad_bnb(dyg, wg, gbuf, rawg, coefs, True, bpart, 1, p, d, addend=None if add is None else nhwc(add))
        dx = ar.grad if add is None else ar.grad + add
        g_ref = dx * (raw * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) > 0)
        close(gbuf, g_ref, 1e-4, 1e-4, "g = relumask * dx")
        xhat = ((raw - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)).double()
        sums = bpart.double().sum(0).cpu()
        gk = gbuf.cpu().double()                              # against the kernel's own g: the summation itself must be fp32-exact
        np.testing.assert_allclose(sums[0].numpy(), gk.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-5 * float(gk.abs().sum((0, 2, 3)).max()))
        np.testing.assert_allclose(sums[1].numpy(), (gk * xhat).sum((0, 2, 3)).numpy(), rtol=1e-5,
                                   atol=1e-5 * float((gk * xhat).abs().sum((0, 2, 3)).max()))
    gb2 = ops.new_act(n, cin, h, w, DEV)
    assert ops.conv_dgrad_bnb(dyg, wg, gb2, rawg, coefs, False, bpart, 1, p, d)
    close(gb2, ar.grad, 1e-4, 1e-4, "no ReLU: g = dx")
    # residual form: the mask comes from a stored block output (out = relu(bn(y) + identity)), not from y*scale+shift
    outp = torch.randn(raw.shape, generator=g)
    gb3 = ops.new_act(n, cin, h, w, DEV)
    assert ops.conv_dgrad_bnb(dyg, wg, gb3, rawg, coefs, True, bpart, 1, p, d, out_prev=nhwc(outp))
    g3 = ar.grad * (outp > 0)
    close(gb3, g3, 1e-4, 1e-4, "mask from out_prev")
    gk = gb3.cpu().double()
    sums = bpart.double().sum(0).cpu()
    np.testing.assert_allclose(sums[1].numpy(), (gk * xhat).sum((0, 2, 3)).numpy(), rtol=1e-5,
                               atol=1e-5 * float((gk * xhat).abs().sum((0, 2, 3)).max()))
    if cin % 4 == 0:
        # ... or from that output's ReLU quad mask (one byte per pixel and 4 channels, written by sh_bn_act): bit-identical
        qm = torch.zeros((n, h, w, cin // 4), dtype=torch.uint8)
        bits = (outp > 0).permute(0, 2, 3, 1).reshape(n, h, w, cin // 4, 4).to(torch.uint8)
        qm = (bits[..., 0] | (bits[..., 1] << 1) | (bits[..., 2] << 2) | (bits[..., 3] << 3)).contiguous().to(DEV)
        gb4, bpart4 = ops.new_act(n, cin, h, w, DEV), torch.empty_like(bpart)
        assert ops.conv_dgrad_bnb(dyg, wg, gb4, rawg, coefs, True, bpart4, 1, p, d, out_prev=qm)
        assert torch.equal(gb4, gb3) and torch.equal(bpart4, bpart)


@pytest.mark.parametrize("case", [(2, 16, 16, 64, 128), (1, 24, 16, 96, 64), (2, 32, 32, 256, 64), (1, 16, 48, 128, 512), (4, 16, 16, 2048, 512)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv1x1_deferred_batchnorm_backward_apply(ops, case, mode, monkeypatch):
    """conv(1x1) -> BN [-> +res] [-> ReLU] backward with the SECOND half of the BatchNorm backward evaluated in the loaders of the
    conv's own dgrad and wgrad (ops.DeferredDy: no sh_bn_bwd_apply pass, no dy tensor; Bottleneck conv1 / conv3, resnet.py via
    torchvision) against the materialised sequence: dgamma / dbeta bit-equal (same statistics pass), dx / dW to fp32 rounding of the
    linear form.  mode: 0 no ReLU, 1 mask from the block output, 2 mask recomputed from y."""
    n, h, w, cin, cout = case
    monkeypatch.setattr(ops, "DEFER_RATIO", 1e9)          # the kernels for every shape, not only where the heuristic defers
    g = torch.Generator().manual_seed(sum(case) + mode)
    x = nhwc(torch.randn(n, cin, h, w, generator=g))
    wt = wl(torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5)
    y = ops.new_act(n, cout, h, w, DEV)
    part = ops.conv_partials(n * h * w, cout, DEV)
    ops.conv_fprop(x, wt, None, y, part, 1, 0, 1)
    gamma = (0.5 + torch.rand(cout, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(cout, generator=g)).to(DEV)
    coefs = ops.bn_finalize(part, n * h * w, gamma, beta, 1e-5, 0.1, None, None, cout, DEV, rows=64)
    out = ops.new_act(n, cout, h, w, DEV)
    res = nhwc(torch.randn(n, cout, h, w, generator=g)) if mode == 1 else None
    ops.bn_act(y, coefs, out, mode != 0, res)
    dout = nhwc(torch.randn(n, cout, h, w, generator=g))
    assert ops.lin_ok(x.shape, wt, 1, 0, 1)
    dy, dg, db, dres = ops.bn_backward(dout, out if mode == 1 else None, y, coefs, gamma, mode, want_dres=True)
    dd, dg2, db2, dres2 = ops.bn_backward(dout, out if mode == 1 else None, y, coefs, gamma, mode, want_dres=True, defer=True)
    assert isinstance(dd, ops.DeferredDy)
    assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dres, dres2)
    scale = float(dy.abs().max())
    close(dd.materialize(), dy, 0, 0, "materialised fallback")
    lin = dd.lin.cpu().double()
    v = lambda t: t.view(1, -1, 1, 1)
    dy_lin = v(lin[0]) * dd.g.cpu().double() + v(lin[1]) * (y.cpu().double() - v(lin[2])) + v(lin[3])
    close(dy_lin.float(), dy, 0, 2e-6 * scale, "linear form")
    add = nhwc(torch.randn(n, cin, h, w, generator=g))
    for a in (None, add):
        dx_ref = ops.new_act(n, cin, h, w, DEV)
        ops.conv_dgrad(dy, wt, dx_ref, 1, 0, 1, addend=a)
        dx = ops.new_act(n, cin, h, w, DEV)
        assert ops.conv_dgrad_lin(dd, wt, dx, addend=a)
        close(dx, dx_ref, 0, 3e-6 * float(dx_ref.abs().max()), "dgrad, dy in the loader")
    # ... with the BatchNorm-backward epilogue for the producer of x
    pc = torch.stack([0.2 * torch.randn(cin, generator=g), 0.5 + torch.rand(cin, generator=g), torch.randn(cin, generator=g),
                      0.3 * torch.randn(cin, generator=g)]).to(DEV).contiguous()
    g_ref, g_lin = ops.new_act(n, cin, h, w, DEV), ops.new_act(n, cin, h, w, DEV)
    p_ref, p_lin = (torch.empty((-(-n * h * w // 64), 2, cin), device=DEV) for _ in range(2))
    assert ops.conv_dgrad_bnb(dy, wt, g_ref, x, pc, True, p_ref, 1, 0, 1, addend=add)
    assert ops.conv_dgrad_lin(dd, wt, g_lin, addend=add, bnb=(x, pc, p_lin))
    # a gradient within rounding of 0 at a masked / unmasked boundary does not exist here: the mask depends on x only
    close(g_lin, g_ref, 0, 3e-6 * float(g_ref.abs().max()), "dgrad + producer's BN-backward front half")
    close(p_lin.sum(0), p_ref.sum(0), 0, 3e-5 * float(p_ref.sum(0).abs().max()), "its partial sums")
    dw_ref, dw = torch.empty_like(wt), torch.empty_like(wt)
    ops.conv_wgrad(x, dy, dw_ref, 1, 0, 1)
    ops.conv_wgrad(x, dd, dw, 1, 0, 1)
    close(dw, dw_ref, 0, 3e-6 * float(dw_ref.abs().max()) * (n * h * w) ** 0.5 / 16, "wgrad, dy in the loader")
    ops.conv_wgrad(x, dy, dw_ref, 1, 0, 1, aff=pc)
    ops.conv_wgrad(x, dd, dw, 1, 0, 1, aff=pc)
    close(dw, dw_ref, 0, 3e-6 * float(dw_ref.abs().max()) * (n * h * w) ** 0.5 / 16, "wgrad, both operands through their BatchNorms")


@pytest.mark.parametrize("case", [(2, 32, 32, 256, 64, 1, 1, 0, 1), (2, 32, 32, 64, 128, 3, 1, 1, 1), (2, 32, 32, 560, 512, 1, 1, 0, 1),
                                  (1, 64, 64, 128, 256, 1, 2, 0, 1), (2, 16, 16, 256, 256, 3, 1, 2, 2)])
def test_conv_bf16_stored_input_three_product_plan(ops, case):
    """A conv whose input is a STORED bf16 tensor read as is (the conv1 / downsample convs of a bf16-stored trunk) runs three MFMA
    products per tile instead of six (the operand's mid / lo planes are zero): output, BatchNorm statistics partials and the weight
    gradient are BIT-identical to the six-product kernels on the same values held as fp32."""
    n, h, w, cin, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(cin + k)
    xb = nhwc(torch.randn(n, cin, h, w, generator=g)).to(torch.bfloat16)
    xf = xb.float()
    wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
    ho, wo = ops.conv_out_hw(h, w, k, k, stride, pad, dil)
    ya, yb_ = ops.new_act(n, cout, ho, wo, DEV), ops.new_act(n, cout, ho, wo, DEV)
    pa, pb = ops.conv_partials(n * ho * wo, cout, DEV), ops.conv_partials(n * ho * wo, cout, DEV)
    ops.conv_fprop(xf, wt, None, ya, pa, stride, pad, dil)
    ops.conv_fprop(xb, wt, None, yb_, pb, stride, pad, dil)
    assert torch.equal(ya, yb_) and torch.equal(pa, pb)
    dy = nhwc(torch.randn(n, cout, ho, wo, generator=g))
    dwa, dwb = torch.empty_like(wt), torch.empty_like(wt)
    ops.conv_wgrad(xf, dy, dwa, stride, pad, dil)
    ops.conv_wgrad(xb, dy, dwb, stride, pad, dil)
    assert torch.equal(dwa, dwb)


def test_conv_reads_and_writes_channel_slices(ops):
    g = torch.Generator().manual_seed(5)
    big_in = nhwc(torch.randn(2, 96, 10, 10, generator=g))
    big_out = ops.new_act(2, 80, 10, 10, DEV, zero=True)
    wt = torch.randn(32, 64, 1, 1, generator=g) / 8
    ops.conv_fprop(big_in[:, 32:96], wl(wt), None, big_out[:, 16:48], None, 1, 0, 1)
    ref = F.conv2d(big_in[:, 32:96].cpu(), wt)
    close(big_out[:, 16:48], ref, 2e-5, 2e-5)
    assert float(big_out[:, :16].abs().max()) == 0 and float(big_out[:, 48:].abs().max()) == 0


@pytest.mark.parametrize("shape,dil", [((2, 64, 16, 16), 1), ((2, 64, 16, 16), 12), ((2, 32, 16, 16), 24),
                                       ((2, 560, 9, 11), 1), ((1, 8, 5, 7), 2), ((2, 72, 16, 24), 1), ((3, 64, 8, 8), 1),
                                       ((1, 136, 16, 40), 1)])
def test_dwconv(ops, shape, dil):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + dil)
    x = torch.randn(shape, generator=g).requires_grad_(True)
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).requires_grad_(True)
    ref = F.conv2d(x, wt, None, 1, dil, dil, groups=c)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    xg, wg = nhwc(x.detach()), wt.detach().to(DEV).contiguous()
    y = ops.new_act(n, c, h, w, DEV)
    part = torch.empty((ops.dw_partials_rows(n, h, w), 2, c), device=DEV)
    ops.dwconv_fprop(xg, wg, y, part, dil)
    close(y, ref, 1e-5, 1e-5)
    coefs = ops.bn_finalize(part, n * h * w, None, None, 1e-5, 0.1, None, None, c, DEV, rows=64)
    close(coefs[0], ref.detach().mean((0, 2, 3)), 1e-4, 1e-5)
    close(coefs[1], 1.0 / torch.sqrt(ref.detach().var((0, 2, 3), unbiased=False) + 1e-5), 1e-4, 1e-5)
    dx = ops.new_act(n, c, h, w, DEV)
    ops.dwconv_dgrad(nhwc(dy), wg, dx, dil)
    close(dx, x.grad, 1e-5, 1e-5)
    ops.dwconv_dgrad(nhwc(dy), wg, dx, dil, accumulate=True)
    close(dx, 2 * x.grad, 1e-5, 2e-5)
    dw = torch.empty_like(wg)
    ops.dwconv_wgrad(xg, nhwc(dy), dw, dil)
    close(dw, wt.grad, 1e-4, 1e-4)


@pytest.mark.parametrize("shape,dil", [((2, 64, 16, 16), 1), ((2, 64, 16, 16), 12), ((1, 72, 9, 11), 1), ((2, 128, 24, 16), 1),
                                       ((1, 136, 16, 40), 1)])
def test_dwconv_fused_batchnorm_hooks(ops, shape, dil):
    """Depthwise conv reading its input through the producer's BatchNorm + ReLU (fprop, wgrad) and emitting the producer's
    BatchNorm-backward statistics + mask from its dgrad epilogue (sep_aspp_contrast_head.py:56-61, 200-203) against torch."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + dil + h)
    raw = torch.randn(shape, generator=g)
    scale, shift = torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    mean, invstd = 0.2 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    coefs = torch.stack([mean, invstd, scale, shift]).to(DEV).contiguous()
    v = lambda t: t.view(1, -1, 1, 1)
    act = torch.relu(raw * v(scale) + v(shift)).requires_grad_(True)
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).requires_grad_(True)
    ref = F.conv2d(act, wt, None, 1, dil, dil, groups=c)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    rawg, wg, dyg = nhwc(raw), wt.detach().to(DEV).contiguous(), nhwc(dy)
    y = ops.new_act(n, c, h, w, DEV)
    part = torch.empty((ops.dw_partials_rows(n, h, w), 2, c), device=DEV)
    ops.dwconv_fprop(rawg, wg, y, part, dil, aff=coefs)
    close(y, ref, 1e-5, 1e-5, "fprop through BN+ReLU")
    dw = torch.empty_like(wg)
    ops.dwconv_wgrad(rawg, dyg, dw, dil, aff=coefs)
    close(dw, wt.grad, 1e-4, 1e-4 * float(wt.grad.abs().max()), "wgrad through BN+ReLU")
    gbuf = ops.new_act(n, c, h, w, DEV)
    bpart = torch.empty((ops.dw_partials_rows(n, h, w), 2, c), device=DEV)
    ops.dwconv_dgrad_bnb(dyg, wg, gbuf, rawg, coefs, bpart, dil)
    g_ref = act.grad * (raw * v(scale) + v(shift) > 0)
    close(gbuf, g_ref, 1e-5, 1e-5, "g = relumask * dx")
    xhat = (raw - v(mean)) * v(invstd)
    sums = bpart.double().sum(0).cpu()
    gk = gbuf.cpu().double()                                  # against the kernel's own g: the summation itself must be fp32-exact
    np.testing.assert_allclose(sums[0].numpy(), gk.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-5 * float(gk.abs().sum((0, 2, 3)).max()))
    np.testing.assert_allclose(sums[1].numpy(), (gk * xhat.double()).sum((0, 2, 3)).numpy(), rtol=1e-5,
                               atol=1e-5 * float((gk * xhat.double()).abs().sum((0, 2, 3)).max()))



@pytest.mark.parametrize("shape", [(2, 64, 16, 16), (1, 136, 16, 40), (2, 128, 24, 16)])
def test_dwconv_deferred_batchnorm_backward_apply(ops, shape):
    """Depthwise dgrad / dgrad+BNB / wgrad with their dy operand evaluated in the loader from (g, y, lin) (ops.DeferredDy: the second
    half of the depthwise conv's own BatchNorm backward, sep_aspp_contrast_head.py:43-61) against the same kernels on the
    materialised dy."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + h)
    gm, y = nhwc(torch.randn(shape, generator=g)), nhwc(torch.randn(shape, generator=g))
    lin = torch.stack([0.5 + torch.rand(c, generator=g), 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g),
                       0.1 * torch.randn(c, generator=g)]).to(DEV).contiguous()
    v = lambda t: t.view(1, -1, 1, 1)
    dy = nhwc((v(lin[0]) * gm + v(lin[1]) * (y - v(lin[2])) + v(lin[3])).cpu())
    dd = ops.DeferredDy(gm, y, lin, None, None, None)
    assert ops.dw_lin_ok(shape, 1)
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).to(DEV).contiguous()
    x = nhwc(torch.randn(shape, generator=g))
    a, b = ops.new_act(n, c, h, w, DEV), ops.new_act(n, c, h, w, DEV)
    ops.dwconv_dgrad(dy, wt, a, 1)
    ops.dwconv_dgrad(dd, wt, b, 1)
    tol = 3e-6 * float(a.abs().max())
    close(b, a, 0, tol, "dgrad")
    pc = torch.stack([0.2 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g), torch.randn(c, generator=g),
                      0.3 * torch.randn(c, generator=g)]).to(DEV).contiguous()
    pa, pb = (torch.empty((ops.dw_partials_rows(n, h, w), 2, c), device=DEV) for _ in range(2))
    ops.dwconv_dgrad_bnb(dy, wt, a, x, pc, pa, 1)
    ops.dwconv_dgrad_bnb(dd, wt, b, x, pc, pb, 1)
    close(b, a, 0, tol, "dgrad + producer's BN-backward front half")
    close(pb.sum(0), pa.sum(0), 0, 3e-5 * float(pa.sum(0).abs().max()), "its partial sums")
    dwa, dwb = torch.empty_like(wt), torch.empty_like(wt)
    ops.dwconv_wgrad(x, dy, dwa, 1)
    ops.dwconv_wgrad(x, dd, dwb, 1)
    close(dwb, dwa, 0, 1e-5 * float(dwa.abs().max()), "wgrad")
    ops.dwconv_wgrad(x, dy, dwa, 1, aff=pc)
    ops.dwconv_wgrad(x, dd, dwb, 1, aff=pc)
    close(dwb, dwa, 0, 1e-5 * float(dwa.abs().max()), "wgrad, x through its BatchNorm")


@pytest.mark.parametrize("operand", ["plain", "aff", "deferred", "aff+deferred"])
def test_weight_gradients_on_the_side_stream_equal_inline(ops, operand):
    """conv_wgrad, _wgrad_b16 and dwconv_wgrad launched on the weight-gradient side stream (side=True, then join_wgrad) give
    BIT-identical weight gradients to the same calls run in order on the compute stream: plain operands, x read through its
    producer's BatchNorm + ReLU (aff=), dy as a DeferredDy, and both."""
    assert ops.WGRAD_ASYNC
    g = torch.Generator().manual_seed(len(operand))
    n, h, w, cin, cout = 2, 16, 16, 64, 128
    aff = "aff" in operand
    deferred = "deferred" in operand
    rnd = lambda *s: torch.randn(*s, generator=g)
    coefs = lambda c: torch.stack([0.2 * rnd(c), 0.5 + torch.rand(c, generator=g), rnd(c), 0.3 * rnd(c)]).to(DEV).contiguous()
    lin = lambda c: torch.stack([0.5 + torch.rand(c, generator=g), 0.3 * rnd(c), 0.2 * rnd(c), 0.1 * rnd(c)]).to(DEV).contiguous()

    def both(run, like):
        a, b = torch.empty_like(like), torch.empty_like(like)
        run(a, False)
        run(b, True)
        ops.join_wgrad()
        torch.cuda.synchronize()
        assert torch.equal(a, b), operand

    # fp32-accurate dense conv: 1x1 (the deferred / loader paths) and 3x3 (the plain and aff paths)
    x = nhwc(rnd(n, cin, h, w))
    pc = coefs(cin) if aff else None
    dy = nhwc(rnd(n, cout, h, w))
    if deferred:
        dy = ops.DeferredDy(dy, nhwc(rnd(n, cout, h, w)), lin(cout), None, None, None)
    like = wl(torch.empty(cout, cin, 1, 1))
    both(lambda dw, side: ops.conv_wgrad(x, dy, dw, 1, 0, 1, side=side, aff=pc), like)
    if not deferred:
        like3 = wl(torch.empty(cout, cin, 3, 3))
        both(lambda dw, side: ops.conv_wgrad(x, dy, dw, 1, 1, 1, side=side, aff=pc), like3)
    # bf16 compute mode
    xb = nhwc_bf16(rnd(n, cin, h, w))
    gb = nhwc_bf16(rnd(n, cout, h, w))
    dyb = ops.DeferredDy(gb, nhwc_bf16(rnd(n, cout, h, w)), lin(cout), None, None, None) if deferred else gb

    def b16(dw, side, pad):
        assert ops._wgrad_b16(xb, dyb, dw, 1, pad, 1, side, pc)
    both(lambda dw, side: b16(dw, side, 0), like)
    if not deferred:
        both(lambda dw, side: b16(dw, side, 1), like3)
    # depthwise (strip-walk kernels)
    c = 128
    xd = nhwc(rnd(n, c, h, w))
    pcd = coefs(c) if aff else None
    dyd = nhwc(rnd(n, c, h, w))
    if deferred:
        dyd = ops.DeferredDy(dyd, nhwc(rnd(n, c, h, w)), lin(c), None, None, None)
    both(lambda dw, side: ops.dwconv_wgrad(xd, dyd, dw, 1, side=side, aff=pcd), torch.empty((c, 1, 3, 3), device=DEV))


def test_side_stream_workspace_is_not_reused_by_the_compute_stream(ops):
    """A side-stream weight gradient whose workspace is replaced by a larger one (the grow-only ops.workspace) while it is still
    queued behind other side-stream work: the retired block must not be handed to a compute-stream allocation before the side
    stream has passed its last use.  Before the workspace was allocated with the side stream as its owner, the allocator returned
    it to the compute stream's pool at once: the probe below received the same block and the wgrad's partial slabs overwrote it."""
    assert ops.WGRAD_ASYNC
    from seghiero_amd._lib import LIB
    c, h, w = 256, 64, 64
    nbytes = lambda n: LIB.raw("sh_dw_partials")(n, h, w) * 9 * c * 4
    small = nbytes(2)
    assert small > 1 << 20 and nbytes(4) > small       # no 1 MiB minimum rounding: the first launch writes its whole buffer
    g = torch.Generator().manual_seed(5)
    x1, dy1 = nhwc(torch.randn(2, c, h, w, generator=g)), nhwc(torch.randn(2, c, h, w, generator=g))
    x2, dy2 = nhwc(torch.randn(4, c, h, w, generator=g)), nhwc(torch.randn(4, c, h, w, generator=g))
    wt = lambda: torch.empty((c, 1, 3, 3), device=DEV)
    ref1, ref2, dw1, dw2 = wt(), wt(), wt(), wt()
    ops.dwconv_wgrad(x2, dy2, dw2, 1, side=True)        # (creates the side stream)
    ops.join_wgrad()
    torch.cuda.synchronize()
    ops._WS.clear()                                      # fresh grow-only workspaces from here on
    side = ops._SIDE[torch.device(DEV).index]
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000_000)                   # holds the side stream for tens of milliseconds
    ops.dwconv_wgrad(x1, dy1, dw1, 1, side=True)        # first workspace: written once the sleep has ended
    (retired,) = [b for k, b in ops._WS.items() if k[1] == "dwwgrad"]
    lo, hi = retired.data_ptr(), retired.data_ptr() + retired.numel()
    assert retired.numel() == small
    del retired
    ops.dwconv_wgrad(x2, dy2, dw2, 1, side=True)        # grows the workspace: the first one is retired
    probe = torch.empty(small, dtype=torch.uint8, device=DEV)       # the compute stream is not waiting for the side stream
    probe.fill_(0x5A)
    p0 = probe.data_ptr()
    assert p0 + small <= lo or p0 >= hi, "a compute-stream tensor was handed the retired side-stream workspace"
    ops.join_wgrad()
    torch.cuda.synchronize()
    assert bool((probe == 0x5A).all()), "the retired workspace was written after the compute stream reused it"
    ops.dwconv_wgrad(x1, dy1, ref1, 1)
    ops.dwconv_wgrad(x2, dy2, ref2, 1)
    assert torch.equal(dw1, ref1) and torch.equal(dw2, ref2)


@pytest.mark.parametrize("shape", [(4, 64, 12, 12), (2, 9, 7, 5), (16, 32, 1, 1)])
@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, False)])
def test_batchnorm_train_fwd_bwd(ops, shape, relu, res):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c)
    y = (torch.randn(shape, generator=g) * 2 + 0.5).requires_grad_(True)
    gamma = (0.5 + torch.rand(c, generator=g)).requires_grad_(True)
    beta = (0.2 * torch.randn(c, generator=g)).requires_grad_(True)
    resid = torch.randn(shape, generator=g).requires_grad_(True) if res else None
    rm, rv = torch.zeros(c), torch.ones(c)
    ref = F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, 1e-5)
    if res:
        ref = ref + resid
    if relu:
        ref = F.relu(ref)
    dout = torch.randn(shape, generator=g)
    ref.backward(dout)
    yg = nhwc(y.detach())
    part = ops.channel_stats(yg)
    rmg, rvg = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    coefs = ops.bn_finalize(part, n * h * w, gamma.detach().to(DEV), beta.detach().to(DEV), 1e-5, 0.1, rmg, rvg, c, DEV, rows=256)
    out = ops.new_act(n, c, h, w, DEV)
    ops.bn_act(yg, coefs, out, relu, None if not res else nhwc(resid.detach()))
    close(out, ref, 1e-5, 2e-5, "bn fwd")
    close(rmg, rm, 1e-5, 1e-6, "running_mean")
    close(rvg, rv, 1e-5, 1e-6, "running_var")
    dy, dgamma, dbeta, dres = ops.bn_backward(nhwc(dout), out if relu else None, yg, coefs, gamma.detach().to(DEV), relu, want_dres=res)
    close(dy, y.grad, 1e-4, 2e-5, "bn dy")
    if relu and not res:      # mode 2: mask recomputed from y and the forward coefficients -- bit-identical to mode 1
        dy2, dg2, db2, _ = ops.bn_backward(nhwc(dout), None, yg, coefs, gamma.detach().to(DEV), 2)
        assert torch.equal(dy2, dy) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    close(dgamma, gamma.grad, 1e-4, 1e-4, "dgamma")
    close(dbeta, beta.grad, 1e-4, 1e-4, "dbeta")
    if res:
        close(dres, resid.grad, 1e-6, 1e-6, "dres")


@pytest.mark.parametrize("c,m,rows", [(64, 16 * 128 * 128, 64), (48, 16 * 128 * 128 - 37, 64), (560, 4100 * 64 - 5, 64), (12, 300000, 64), (9, 300000, 64)])
def test_batchnorm_fold_partials_before_finalize(ops, c, m, rows, monkeypatch):
    """Long statistics lists are folded 64:1 (sh_bn_fold_partials: centred merge in f64, same partial format) before the finalize
    kernels: coefficients / running statistics (forward) and dgamma / dbeta / c1 / c2 (backward) equal those of the one-stage
    finalize of the full list to fp32 rounding of the folded partials (1e-6 relative), and an f64 reference; ragged tails (last
    partial short, last chunk short) and a channel count that is no multiple of 32 included."""
    g = torch.Generator(device=DEV).manual_seed(c)
    p = -(-m // rows)
    # centred partials of random data: per partial (sum, M2 about its own mean) of n_p values ~ N(mu_c, sd_c) -- built in f64
    n_p = torch.full((p,), rows, device=DEV, dtype=torch.float64); n_p[-1] = m - (p - 1) * rows
    mu = torch.linspace(-3, 5, c, device=DEV, dtype=torch.float64)
    mean_p = mu[None, :] + 0.3 * torch.randn((p, c), generator=g, device=DEV, dtype=torch.float64)
    m2_p = (0.5 + torch.rand((p, c), generator=g, device=DEV, dtype=torch.float64)) * n_p[:, None]
    part = torch.stack([mean_p * n_p[:, None], m2_p], 1).float().contiguous()
    s64, q64 = part[:, 0].double(), part[:, 1].double()
    tot = s64.sum(0)
    mean_ref = tot / m
    var_ref = (q64 + s64 * s64 / n_p[:, None]).sum(0) / m - mean_ref ** 2
    gamma, beta = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)

    def fwd(fold_min):
        monkeypatch.setattr(ops, "FOLD_MIN", fold_min)
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        return ops.bn_finalize(part, m, gamma, beta, 1e-5, 0.1, rm, rv, c, DEV, rows=rows).clone(), rm, rv
    (c0, rm0, rv0), (c1, rm1, rv1) = fwd(1 << 30), fwd(1024)
    if c % 4 == 0:          # (else sh_bn_fold_partials answers SH_EUNSUPPORTED and the list is finalized as it is: bit-equal)
        close(c1[0], mean_ref.float(), 1e-6, 1e-6, "mean vs f64")
        close(c1[1], (1.0 / torch.sqrt(var_ref + 1e-5)).float(), 2e-6, 0, "invstd vs f64")
    close(c1, c0, 2e-6, 1e-6, "folded vs one-stage coefficients")
    close(rm1, rm0, 2e-6, 1e-7); close(rv1, rv0, 2e-6, 1e-7)
    # backward: plain sums
    bp = torch.randn((p, 2, c), generator=g, device=DEV) * 3

    def bwd(fold_min):
        monkeypatch.setattr(ops, "FOLD_MIN", fold_min)
        red = torch.empty((4, c), device=DEV)
        q, _ = ops._fold_partials(bp, c, m, 0)
        assert q.shape[0] == (p if (fold_min > p or c % 4) else -(-p // 64))
        ops._call("sh_bn_bwd_finalize", q.data_ptr(), q.shape[0], c, gamma.data_ptr(), c0[1].data_ptr(), float(m),
                  red[0].data_ptr(), red[1].data_ptr(), red[2].data_ptr(), red[3].data_ptr(), c0[0].data_ptr(), None, ops._st())
        return red
    r0, r1 = bwd(1 << 30), bwd(1024)
    ref = bp.double().sum(0)
    scale = float(bp.abs().max()) * (p ** 0.5)
    close(r1[1], ref[0].float(), 0, 2e-6 * scale, "dbeta vs f64")
    close(r1[0], ref[1].float(), 0, 2e-6 * scale, "dgamma vs f64")
    close(r1, r0, 0, 2e-6 * scale, "folded vs one-stage backward sums")


def test_relu_quad_mask_stands_in_for_the_block_output(ops):
    """sh_bn_act's relu_mask output is bit j = (out[c + j] > 0) per (pixel, channel quad), and the BatchNorm backward fed the mask
    (relu = 3) is bit-identical to the one fed the output itself (relu = 1): statistics pass, its stored masked gradient, apply pass."""
    n, c, h, w = 3, 40, 9, 7
    g = torch.Generator().manual_seed(11)
    y, res, dout = nhwc(torch.randn(n, c, h, w, generator=g)), nhwc(torch.randn(n, c, h, w, generator=g)), nhwc(torch.randn(n, c, h, w, generator=g))
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    coefs = ops.bn_finalize(ops.channel_stats(y), n * h * w, gamma, beta, 1e-5, 0.1, rm, rv, c, DEV, rows=256)
    out, mask = ops.new_act(n, c, h, w, DEV), ops.new_relu_mask(n, c, h, w, DEV)
    ops.bn_act(y, coefs, out, True, res, mask=mask)
    bits = (out > 0).permute(0, 2, 3, 1).reshape(n, h, w, c // 4, 4).to(torch.uint8)
    assert torch.equal(mask, bits[..., 0] | (bits[..., 1] << 1) | (bits[..., 2] << 2) | (bits[..., 3] << 3))
    for defer in (False, True):
        a = ops.bn_backward(dout, out, y, coefs, gamma, 1, want_dres=True, defer=defer)
        b = ops.bn_backward(dout, mask, y, coefs, gamma, 1, want_dres=True, defer=defer)
        da = a[0].materialize() if hasattr(a[0], "materialize") else a[0]
        db = b[0].materialize() if hasattr(b[0], "materialize") else b[0]
        assert torch.equal(da, db) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_bn_eval_coefs(ops):
    g = torch.Generator().manual_seed(1)
    c = 24
    y = torch.randn(2, c, 5, 5, generator=g)
    gamma, beta, rm, rv = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    ref = F.batch_norm(y, rm, rv, gamma, beta, False, 0.1, 1e-5)
    coefs = ops.bn_eval_coefs(gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), 1e-5)
    out = ops.new_act(2, c, 5, 5, DEV)
    ops.bn_act(nhwc(y), coefs, out, False)
    close(out, ref, 1e-5, 1e-5)


@pytest.mark.parametrize("shape", [(2, 64, 32, 32), (2, 8, 15, 17)])
def test_maxpool(ops, shape):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g)
    x[0, :, 2:6, 2:6] = 1.0          # ties: first max in row-major order takes the gradient
    x.requires_grad_(True)
    ref = F.max_pool2d(x, 3, 2, 1)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    xg = nhwc(x.detach())
    y, am = ops.maxpool_fwd(xg)
    assert torch.equal(y.cpu(), ref.detach())
    dx = ops.maxpool_bwd(am, nhwc(dy), xg.shape[2], xg.shape[3])
    close(dx, x.grad, 1e-6, 1e-6)


def test_avgpool_broadcast(ops):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 40, 16, 16, generator=g)
    y = ops.avgpool_fwd(nhwc(x))
    close(y, F.adaptive_avg_pool2d(x, 1), 1e-6, 1e-6)
    out = ops.new_act(3, 100, 6, 5, DEV, zero=True)
    ops.broadcast_hw(y, out[:, 20:60])
    close(out[:, 20:60], F.interpolate(F.adaptive_avg_pool2d(x, 1), size=(6, 5), mode="bilinear", align_corners=False), 1e-6, 1e-6)
    dy = torch.randn(3, 40, 6, 5, generator=g)
    close(ops.sum_hw(nhwc(dy)), dy.sum((2, 3), keepdim=True), 1e-5, 1e-5)
    dx = nhwc(x.clone())
    ops.avgpool_bwd(y, dx, accumulate=True)
    close(dx, x + F.adaptive_avg_pool2d(x, 1) / 256, 1e-6, 1e-6)


@pytest.mark.parametrize("src,dst", [((16, 16), (128, 128)), ((3, 2), (19, 13)), ((4, 4), (32, 32)), ((8, 8), (8, 8)), ((10, 12), (5, 6))])
def test_bilinear(ops, src, dst):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, *src, generator=g).requires_grad_(True)
    ref = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    out = ops.new_act(2, 16, *dst, DEV)
    ops.bilinear_fwd(nhwc(x.detach()), out)
    close(out, ref, 1e-5, 1e-6)
    dx = ops.bilinear_bwd(nhwc(dy), *src)
    close(dx, x.grad, 1e-5, 1e-5)


def test_l2norm(ops):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 40, 5, 6, generator=g).requires_grad_(True)
    ref = F.normalize(x, p=2, dim=1)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    y, norm = ops.l2norm_fwd(nhwc(x.detach()))
    close(y, ref, 1e-6, 1e-6)
    close(ops.l2norm_bwd(nhwc(dy), y, norm), x.grad, 1e-5, 1e-6)


def test_layout_roundtrip(ops):
    x = torch.randn(2, 3, 9, 7)
    y = ops.to_nhwc(x.to(DEV), cpad=4)
    assert ops.pm(y)[1] == 4
    assert torch.equal(y.cpu(), x)


def test_sgd(ops):
    g = torch.Generator().manual_seed(8)
    shapes = [(7,), (64, 3, 7, 7), (13, 512, 1, 1), (1001,)] * 20          # 80 tensors -> two launches
    ps = [torch.randn(s, generator=g) for s in shapes]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.SGD(ref, lr=0.05, momentum=0.9, weight_decay=1e-4)
    gp = [p.to(DEV) for p in ps]
    bufs = [torch.zeros_like(p) for p in gp]
    for step in range(3):
        grads = [torch.randn(s, generator=g) for s in shapes]
        for r, gr in zip(ref, grads):
            r.grad = gr.clone()
        opt.step()
        ops.sgd_step(gp, [gr.to(DEV) for gr in grads], bufs, 0.05, 0.9, 1e-4, step == 0)
    for a, b in zip(gp, ref):
        close(a, b, 1e-6, 1e-6)


@pytest.mark.parametrize("resize", [None, (40, 28)])
def test_ingest_matches_reference_transform_arithmetic(ops, resize):
    """flip + ToTensor + Normalize + nearest mask resize (dataset/dataloader.py:49-63) on the device,
    against the same steps in torch on the CPU -- bit-exact for the image (same operation order) and the labels."""
    from seghiero_amd.ingest import JointTransformDevice
    g = torch.Generator().manual_seed(3)
    n, h, w = 5, 28, 40                       # resize is (W, H) as in PIL
    rgb = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    hs, ws = (h, w) if resize is None else (61, 47)
    mask = torch.randint(0, 9, (n, hs, ws), generator=g)
    mask[0, :3] = 255
    tf = JointTransformDevice(resize=resize, hflip_prob=0.5)
    img, lab = tf(rgb.to(DEV), mask.to(DEV), generator=torch.Generator().manual_seed(11))
    flip = torch.rand(n, generator=torch.Generator().manual_seed(11)) < 0.5
    assert flip.any() and not flip.all()
    mean, std = torch.tensor(tf.normalize_mean).view(1, 3, 1, 1), torch.tensor(tf.normalize_std).view(1, 3, 1, 1)
    ref = rgb.permute(0, 3, 1, 2).float().div(255)             # ToTensor
    m = mask
    if resize is not None:
        m = F.interpolate(mask[:, None].float(), size=(h, w), mode="nearest").long()[:, 0]
    ref = torch.where(flip.view(n, 1, 1, 1), ref.flip(3), ref)
    m = torch.where(flip.view(n, 1, 1), m.flip(2), m)
    ref = (ref - mean) / std                                     # Normalize
    assert tuple(img.shape) == (n, 4, h, w) and img.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(img[:, :3].cpu(), ref)
    assert float(img[:, 3].abs().max()) == 0.0
    assert lab.dtype == torch.uint8 and torch.equal(lab.cpu().long(), m)


@pytest.mark.parametrize("tag", ["down", "up", "mixed", "big", "same_w"])
def test_pil_bilinear_resize_bit_exact(ops, tag):
    """SURVEY 8f row 3 / dataset/dataloader.py:50: `img.resize(size, Image.BILINEAR)` on the device, bit-identical to the arrays
    Pillow itself produced (tests/golden/g9_pil_bilinear.npz, tools/make_goldens.py g9); batch of two (second image flipped)."""
    from conftest import load_golden
    from seghiero_amd.ingest import JointTransformDevice, resize_bilinear_u8
    g = load_golden("g9_pil_bilinear")
    a, ref = torch.from_numpy(g[f"{tag}_in"]), torch.from_numpy(g[f"{tag}_out"])
    ho, wo = ref.shape[:2]
    got = resize_bilinear_u8(a[None].to(DEV).contiguous(), (wo, ho))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, ho, wo, 3)
    assert torch.equal(got[0].cpu(), ref)
    # the whole transform from an un-resized image: resize -> ToTensor -> Normalize, no flip
    tf = JointTransformDevice(resize=(wo, ho), hflip_prob=0.0)
    mask = torch.zeros(1, a.shape[0], a.shape[1], dtype=torch.long)
    img, lab = tf(a[None].to(DEV).contiguous(), mask.to(DEV))
    mean, std = torch.tensor(tf.normalize_mean).view(1, 3, 1, 1), torch.tensor(tf.normalize_std).view(1, 3, 1, 1)
    want = (ref.permute(2, 0, 1)[None].float().div(255) - mean) / std
    assert torch.equal(img[:, :3].cpu(), want) and tuple(lab.shape) == (1, ho, wo)


def test_backbone_accepts_ingested_input(ops):
    from seghiero_amd.backbone import ResNetBackbone
    torch.manual_seed(0)
    bb = ResNetBackbone(depth=18, pretrained=False).to(DEV).train()
    x = torch.randn(2, 3, 64, 64)
    a = bb(x.to(DEV))
    x4 = ops.new_act(2, 4, 64, 64, DEV, zero=True)
    x4[:, :3] = x.to(DEV)
    bb2 = ResNetBackbone(depth=18, pretrained=False).to(DEV).train()
    bb2.load_state_dict(bb.state_dict())
    b = bb2(x4)
    # running stats were bumped once in each module from the same input: compare the features directly
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_weight_transpose_multi_matches_single(ops):
    g = torch.Generator().manual_seed(9)
    shapes = [(13, 16, 1, 1), (64, 32, 3, 3), (48, 256, 1, 1), (32, 8, 5, 5)] * 12      # 48 weights: two launches
    ws = [wl(torch.randn(s, generator=g)) for s in shapes]
    singles = [ops.weight_transpose(w) for w in ws]
    cache = {}
    ops.prepare_dgrad_weights(ws, cache)
    try:
        for w, ref in zip(ws, singles):
            got = ops.weight_transpose(w)
            assert got.data_ptr() != ref.data_ptr() and torch.equal(got, ref)
    finally:
        ops.release_dgrad_weights()
    bufs = [v[1] for k, v in cache.items() if k != "__plan__"]          # ("__plan__": the launch tables kept with the buffers)
    assert len(bufs) == len(ws)
    assert ops.weight_transpose(ws[0]).data_ptr() not in [t.data_ptr() for t in bufs]
    # a second prepare with the same weights reuses the tables and reproduces the copies
    ops.prepare_dgrad_weights(ws, cache)
    try:
        assert all(torch.equal(ops.weight_transpose(w), ref) for w, ref in zip(ws, singles))
    finally:
        ops.release_dgrad_weights()


def test_layout_and_axpy_helpers(ops):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, 3, 17, 23, generator=g)
    y = ops.new_act(3, 4, 17, 23, DEV)
    ops._call("sh_nchw_to_nhwc", x.to(DEV).data_ptr(), y.data_ptr(), 3, 3, 17, 23, 4, ops._st())
    assert torch.equal(y[:, :3].cpu(), x) and float(y[:, 3].abs().max()) == 0.0
    for n in (1024, 1001):                      # 16-byte path and scalar path
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        ag = a.to(DEV)
        ops._call("sh_axpy", ag.data_ptr(), b.to(DEV).data_ptr(), 0.5, n, ops._st())
        assert torch.equal(ag.cpu(), a + 0.5 * b)


@pytest.mark.parametrize("shape", [(16, 128, 128, 512, 512, 1), (16, 32, 32, 256, 256, 3)])
def test_full_size_conv_properties(ops, shape):
    """BASELINE-size layers (the decoder's 512->512 pointwise at 128^2 x 16 and layer3's 3x3) are too big for a CPU reference in
    the test budget; check size-independent properties instead: exact homogeneity under a power-of-two scale (every rounding
    step scales exactly), batch additivity of the weight gradient, and agreement of a sampled set of outputs with an fp64 dot
    product."""
    n, h, w, cin, cout, k = shape
    g = torch.Generator(device=DEV).manual_seed(1)
    x = ops.new_act(n, cin, h, w, DEV); x.normal_(generator=g)
    wt = (torch.randn(cout, cin, k, k, device=DEV, generator=g) / (cin * k * k) ** 0.5).contiguous(memory_format=torch.channels_last)
    pad = k // 2
    y = ops.new_act(n, cout, h, w, DEV)
    ops.conv_fprop(x, wt, None, y, None, 1, pad, 1)
    x2 = ops.new_act(n, cin, h, w, DEV); x2.copy_(x * 2)
    y2 = ops.new_act(n, cout, h, w, DEV)
    ops.conv_fprop(x2, wt, None, y2, None, 1, pad, 1)
    assert torch.equal(y2, y * 2)
    # sampled outputs against an fp64 evaluation
    idx = torch.randint(0, n * h * w, (64,), generator=torch.Generator().manual_seed(2))
    xp = torch.nn.functional.pad(x.double(), (pad, pad, pad, pad))
    for t in idx.tolist():
        b, r = divmod(t, h * w)
        oy, ox = divmod(r, w)
        patch = xp[b, :, oy:oy + k, ox:ox + k]                              # [cin, k, k]
        ref = (wt.double() * patch[None]).sum((1, 2, 3))
        got = y[b, :, oy, ox].double()
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max() + 1)
    # dgrad homogeneity and wgrad batch additivity
    dy = ops.new_act(n, cout, h, w, DEV); dy.normal_(generator=g)
    dx = ops.new_act(n, cin, h, w, DEV); dx4 = ops.new_act(n, cin, h, w, DEV)
    ops.conv_dgrad(dy, wt, dx, 1, pad, 1)
    dy4 = ops.new_act(n, cout, h, w, DEV); dy4.copy_(dy * 4)
    ops.conv_dgrad(dy4, wt, dx4, 1, pad, 1)
    assert torch.equal(dx4, dx * 4)
    dw, dwa, dwb = torch.empty_like(wt), torch.empty_like(wt), torch.empty_like(wt)
    ops.conv_wgrad(x, dy, dw, 1, pad, 1)
    hb = n // 2
    ops.conv_wgrad(x[:hb], dy[:hb], dwa, 1, pad, 1)
    ops.conv_wgrad(x[hb:], dy[hb:], dwb, 1, pad, 1)
    rel = float((dwa + dwb - dw).norm() / dw.norm())
    assert rel < 2e-6, rel


def test_full_size_batchnorm_statistics(ops):
    """Train-mode BN at a BASELINE-size tensor (16 x 256 x 128 x 128): the normalised output has per-channel mean beta and
    variance gamma^2 (a checksum of the statistics path: centred conv-epilogue style partials -> f64 finalize -> apply)."""
    n, c, h, w = 16, 256, 128, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    y = ops.new_act(n, c, h, w, DEV); y.normal_(generator=g)
    y.mul_(torch.linspace(0.5, 3.0, c, device=DEV).view(1, c, 1, 1)).add_(torch.linspace(-2, 2, c, device=DEV).view(1, c, 1, 1))
    gamma, beta = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    part = ops.channel_stats(y)
    coefs = ops.bn_finalize(part, n * h * w, gamma, beta, 1e-5, 0.1, rm, rv, c, DEV, rows=256)
    out = ops.new_act(n, c, h, w, DEV)
    ops.bn_act(y, coefs, out, False, None)
    m = out.double().mean((0, 2, 3)).float()
    v = out.double().var((0, 2, 3), unbiased=False).float()
    close(m, beta, 0, 2e-5)
    close(v, gamma * gamma, 1e-4, 1e-6)


# ---------------------------------------------------------------------------------------------- bf16 compute mode (csrc/conv_b16.hip)
def nhwc_bf16(t, ld=None):
    """CPU NCHW tensor -> GPU logical-NCHW bf16 tensor with NHWC memory (optionally a channel slice of a wider buffer)."""
    n, c, h, w = t.shape
    ld = c if ld is None else ld
    buf = torch.zeros((n, h, w, ld), device=DEV, dtype=torch.bfloat16)
    out = buf.permute(0, 3, 1, 2)[:, :c]
    out.copy_(t.to(DEV))
    return out


B16_CASES = [
    # n, h, w, cin, cout, k, pad, dil
    (2, 16, 16, 64, 64, 1, 0, 1),          # K = 64: one tile
    (2, 16, 16, 64, 256, 1, 0, 1),
    (2, 24, 16, 256, 64, 1, 0, 1),         # 128 x 64 tiles
    (2, 16, 16, 560, 512, 1, 0, 1),        # K tail: 560 = 8.75 tiles of 64
    (1, 17, 13, 128, 128, 3, 1, 1),        # 3 x 3, rows beyond M, odd sizes
    (2, 12, 12, 64, 64, 3, 1, 1),          # 3 x 3 with Cin = 64: one tile per tap
    (2, 12, 12, 256, 64, 3, 1, 1),         # long K, few tiles: K slices + reduce
    (2, 12, 12, 64, 256, 3, 12, 12),       # dilated
    (4, 16, 16, 2048, 512, 1, 0, 1),       # the ASPP pointwise shape
    (1, 40, 40, 48, 32, 1, 0, 1),          # K = 48 < one tile, Cout = 32
]


@pytest.mark.parametrize("case", B16_CASES)
def test_conv_bf16_compute_mode_matches_exact_products_of_the_rounded_operands(ops, case):
    """bf16 compute mode (sh_conv_fprop_b16 / _dgrad_b16 / _wgrad_b16): operands rounded ONCE to bf16, one MFMA product, fp32 accumulate.
    The reference is therefore exact: fp64 convolutions of the bf16-rounded operands; what remains is the fp32 summation order --
    2e-5 of the result's scale (the fp32-accurate kernels are held to the same figure against fp32 torch).  Forward also through the
    producer's BatchNorm + ReLU in the loader (one fused multiply-add, ReLU, then rounded to bf16), with
    BatchNorm statistics from the fp32 accumulators and a bf16- or fp32-stored output; input gradient with fp32 and bf16 gradient
    operands, addend, BatchNorm-backward epilogue; weight gradient plain and through the loader."""
    n, h, w, cin, cout, k, p, d = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    wq = bf(wt).double()
    scale, shift = torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g)
    mean, invstd = 0.2 * torch.randn(cin, generator=g), 0.5 + torch.rand(cin, generator=g)
    coefs = torch.stack([mean, invstd, scale, shift]).to(DEV).contiguous()
    # the loader's arithmetic: ONE fused multiply-add in fp32 (x is bf16, so the product is exact in fp64 and rounding the fp64 sum to fp32
    # is the fused result)
    pre = (x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float()
    act = bf(torch.relu(pre))
    xg, wg = nhwc_bf16(x), wl(wt)
    ref_plain = F.conv2d(x.double(), wq, None, 1, p, d)
    ref_act = F.conv2d(act.double(), wq, None, 1, p, d)
    ho, wo = ref_plain.shape[2:]
    m = n * ho * wo
    tol = lambda r: dict(rtol=2e-5, atol=2e-5 * float(r.abs().max()))
    with ops.compute_as(torch.bfloat16):
        assert ops.b16()
        # ---- forward: plain and through the loader; fp32 output pins the accumulation, bf16 output is its rounding
        for coef, ref in ((None, ref_plain), (coefs, ref_act)):
            y = ops.new_act(n, cout, ho, wo, DEV, zero=True)
            part = ops.conv_partials(m, cout, DEV)
            assert ops._fprop_b16(xg, coef, wg, None, y, part, 1, p, d), "no bf16 instantiation for a model shape"
            np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), **tol(ref))
            st = ops.bn_finalize(part, m, None, None, 1e-5, 0.1, None, None, cout, DEV, rows=64)
            close(st[0], ref.float().mean((0, 2, 3)), 1e-4, 1e-5, "BatchNorm mean from the fp32 accumulators")
            close(st[1], 1.0 / torch.sqrt(ref.float().var((0, 2, 3), unbiased=False) + 1e-5), 1e-4, 1e-5, "invstd")
            yb = ops.new_act(n, cout, ho, wo, DEV, zero=True, dtype=torch.bfloat16)
            assert ops._fprop_b16(xg, coef, wg, None, yb, None, 1, p, d)
            assert torch.equal(yb, y.to(torch.bfloat16)), "bf16 output = round-to-nearest-even of the fp32 result"
        # ---- input gradient: fp32 and bf16 gradient operands
        dy = torch.randn(n, cout, ho, wo, generator=g)
        dyq = bf(dy)
        ref_dx = torch.nn.grad.conv2d_input((n, cin, h, w), wq, dyq.double(), 1, p, d)
        ldy = ops.pad8(cout)
        dy32 = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
        dy32.copy_(dyq.float().to(DEV))                                                    # fp32 tensor holding bf16-representable values
        dy16 = nhwc_bf16(dyq, ld=ldy)
        for dyt in (dy32, dy16):
            dx = ops.new_act(n, cin, h, w, DEV)
            assert ops._dgrad_b16(dyt, wg, dx, 1, p, d)
            np.testing.assert_allclose(dx.cpu().double().numpy(), ref_dx.numpy(), **tol(ref_dx))
        add = bf(torch.randn(n, cin, h, w, generator=g))
        dxb = ops.new_act(n, cin, h, w, DEV, dtype=torch.bfloat16)
        assert ops._dgrad_b16(dy16, wg, dxb, 1, p, d, addend=nhwc_bf16(add))
        want = (ref_dx + add.double()).float()
        err = (dxb.cpu().double() - want.double()).abs().max() / want.abs().max()
        assert float(err) < 2 ** -8, ("bf16 dx + bf16 addend", float(err))                 # one bf16 rounding of the sum
        # BatchNorm-backward epilogue on a deferred input: g = relumask(y_prev * scale + shift) * dx, partial sums of g and g * xhat
        gbuf = ops.new_act(n, cin, h, w, DEV)
        bpart = torch.empty((-(-n * h * w // 64), 2, cin), device=DEV)
        assert ops._dgrad_b16(dy16, wg, gbuf, 1, p, d, bnb=(xg, coefs, True, bpart, None))
        g_ref = ref_dx * (pre > 0)
        np.testing.assert_allclose(gbuf.cpu().double().numpy(), g_ref.numpy(), **tol(ref_dx))
        xhat = ((x.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1))
        gk = gbuf.cpu().double()
        sums = bpart.double().sum(0).cpu()
        np.testing.assert_allclose(sums[0].numpy(), gk.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-5 * float(gk.abs().sum((0, 2, 3)).max()))
        np.testing.assert_allclose(sums[1].numpy(), (gk * xhat).sum((0, 2, 3)).numpy(), rtol=1e-5,
                                   atol=1e-5 * float((gk * xhat).abs().sum((0, 2, 3)).max()))
        # ... the same with every tensor of the epilogue in bf16 (the bf16-gradient step: all loads of the tile issued up front), mask
        # recomputed from y, and taken from a ReLU quad mask with a bf16 addend
        gb16 = ops.new_act(n, cin, h, w, DEV, dtype=torch.bfloat16)
        bp16 = torch.empty_like(bpart)
        assert ops._dgrad_b16(dy16, wg, gb16, 1, p, d, bnb=(xg, coefs, True, bp16, None))
        e = float((gb16.cpu().double() - g_ref).abs().max() / ref_dx.abs().max())
        assert e < 2 ** -8, ("bf16 g", e)
        np.testing.assert_allclose(bp16.double().sum(0).cpu().numpy(), sums.numpy(), rtol=1e-4, atol=1e-4 * float(gk.abs().sum((0, 2, 3)).max()))
        outp = torch.randn(n, cin, h, w, generator=g)
        bits = (outp > 0).permute(0, 2, 3, 1).reshape(n, h, w, cin // 4, 4).to(torch.uint8)
        qm = (bits[..., 0] | (bits[..., 1] << 1) | (bits[..., 2] << 2) | (bits[..., 3] << 3)).contiguous().to(DEV)
        assert ops._dgrad_b16(dy16, wg, gb16, 1, p, d, addend=nhwc_bf16(add), bnb=(xg, coefs, True, bp16, qm))
        g3 = (ref_dx + add.double()) * (outp > 0)
        e = float((gb16.cpu().double() - g3).abs().max() / g3.abs().max())
        assert e < 2 ** -8, ("bf16 g, quad mask + addend", e)
        s3 = bp16.double().sum(0).cpu()
        np.testing.assert_allclose(s3[1].numpy(), (g3 * xhat).sum((0, 2, 3)).numpy(), rtol=2e-4, atol=2e-4 * float((g3 * xhat).abs().sum((0, 2, 3)).max()))
        # ---- weight gradient: plain and with x through the loader, fp32 and bf16 gradient operands
        if cout % 8 == 0:
            for xin, coef in ((x, None), (act, coefs)):
                ref_dw = torch.nn.grad.conv2d_weight(xin.double(), (cout, cin, k, k), dyq.double(), 1, p, d)
                for dyt in (dy32, dy16):
                    dw = torch.empty_like(wg)
                    assert ops._wgrad_b16(xg, dyt, dw, 1, p, d, False, coef), "no bf16 weight-gradient instantiation for a model shape"
                    np.testing.assert_allclose(dw.cpu().double().numpy(), ref_dw.numpy(), **tol(ref_dw))


@pytest.mark.parametrize("case", [(2, 16, 16, 512, 25), (1, 24, 20, 64, 13), (2, 8, 8, 128, 20)])
def test_conv_bf16_compute_mode_classifier_channel_counts(ops, case):
    """Cout % 8 != 0 (the classifier, 512 -> n_fine) in bf16 compute mode: the forward writes rows of pad8(Cout) (padding lanes zero, bias
    zero-padded by ops), the input gradient and the weight gradient read the loss gradient from rows of pad8(Cout) with zeroed padding."""
    n, h, w, cin, cout = case
    g = torch.Generator().manual_seed(sum(case))
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bias = torch.randn(cout, generator=g)
    wq = bf(wt).double()
    scale, shift = torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g)
    coefs = torch.stack([torch.zeros(cin), torch.ones(cin), scale, shift]).to(DEV).contiguous()
    pre = (x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float()
    act = bf(torch.relu(pre))
    xg, wg, bg = nhwc_bf16(x), wl(wt), bias.to(DEV)
    ld = ops.pad8(cout)
    tol = lambda r: dict(rtol=2e-5, atol=2e-5 * float(r.abs().max()))
    with ops.compute_as(torch.bfloat16):
        for coef, xin in ((None, x), (coefs, act)):
            ref = F.conv2d(xin.double(), wq, bias.double())
            y = ops.new_act(n, cout, h, w, DEV, ld=ld)
            y.fill_(float("nan"))
            assert ops._fprop_b16(xg, coef, wg, bg, y, None, 1, 0, 1), "no bf16 instantiation for the classifier"
            np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), **tol(ref))
            full = torch.as_strided(y, (n, h, w, ld), (h * w * ld, w * ld, ld, 1))
            assert torch.equal(full[..., cout:], torch.zeros_like(full[..., cout:])), "padding lanes of the logits rows are written as zeros"
        dyq = bf(torch.randn(n, cout, h, w, generator=g))
        dy32 = ops.new_act(n, cout, h, w, DEV, ld=ld, zero=True)
        dy32.copy_(dyq.float().to(DEV))
        ref_dx = torch.nn.grad.conv2d_input((n, cin, h, w), wq, dyq.double())
        for dxdt in (torch.float32, torch.bfloat16):
            dx = ops.new_act(n, cin, h, w, DEV, dtype=dxdt)
            assert ops._dgrad_b16(dy32, wg, dx, 1, 0, 1)
            e = float((dx.cpu().double() - ref_dx).abs().max() / ref_dx.abs().max())
            assert e < (2e-5 if dxdt == torch.float32 else 2 ** -8), (dxdt, e)
        for xin, coef in ((x, None), (act, coefs)):
            ref_dw = torch.nn.grad.conv2d_weight(xin.double(), (cout, cin, 1, 1), dyq.double())
            dw = torch.empty_like(wg)
            assert ops._wgrad_b16(xg, dy32, dw, 1, 0, 1, False, coef), "no bf16 weight-gradient instantiation for the classifier"
            np.testing.assert_allclose(dw.cpu().double().numpy(), ref_dw.numpy(), **tol(ref_dw))


B16_STRIDED = [
    # n, h, w, cin, cout, k, pad
    (2, 16, 16, 128, 128, 3, 1),           # layer2.0.conv2's plan: 3 x 3 stride 2, four parity classes
    (1, 17, 13, 64, 64, 3, 1),             # odd sizes: classes of different extent, rows beyond the smaller classes
    (2, 12, 20, 32, 64, 3, 1),             # 128 x 64 tiles (Cin = 32)
    (2, 16, 16, 256, 512, 1, 0),           # the downsample branch: 1 x 1 stride 2, added into dx at the even pixels
    (1, 15, 11, 64, 128, 1, 0),            # odd sizes
]


@pytest.mark.parametrize("case", B16_STRIDED)
def test_conv_bf16_compute_mode_strided_input_gradients(ops, case):
    """Input gradients of the strided convs in bf16 compute mode (conv_b16_kernel's row maps): stride-2 K x K by input-parity class and
    the 1 x 1 strided conv whose result is ADDED to an existing dx at the strided pixels (sh_conv_dgrad_b16 act_flags bit 6) -- against
    fp64 gradients of the bf16-rounded operands, fp32 and bf16 gradient operand, fp32 and bf16 result (one rounding of the sum)."""
    n, h, w, cin, cout, k, p = case
    g = torch.Generator().manual_seed(sum(case) + 7)
    bf = lambda t: t.to(torch.bfloat16)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cout * k * k) ** 0.5
    wq, wg = bf(wt).double(), wl(wt)
    ho, wo = (h + 2 * p - k) // 2 + 1, (w + 2 * p - k) // 2 + 1
    dyq = bf(torch.randn(n, cout, ho, wo, generator=g))
    ref = torch.nn.grad.conv2d_input((n, cin, h, w), wq, dyq.double(), 2, p, 1)
    ldy = ops.pad8(cout)
    dy32 = ops.new_act(n, cout, ho, wo, DEV, ld=ldy, zero=True)
    dy32.copy_(dyq.float().to(DEV))
    dy16 = nhwc_bf16(dyq, ld=ldy)
    tol = dict(rtol=2e-5, atol=2e-5 * float(ref.abs().max()))
    scatter = k == 1
    base = bf(torch.randn(n, cin, h, w, generator=g))               # what dx holds before the scatter-add
    with ops.compute_as(torch.bfloat16):
        for dyt in (dy32, dy16):
            dx = ops.new_act(n, cin, h, w, DEV)
            if scatter:
                dx.copy_(base.float().to(DEV))
            else:
                dx.fill_(float("nan"))                               # every pixel belongs to exactly one class and is written
            assert ops._dgrad_b16(dyt, wg, dx, 2, p, 1, scatter=scatter), "no bf16 instantiation for a model shape"
            want = ref + base.double() if scatter else ref
            np.testing.assert_allclose(dx.cpu().double().numpy(), want.numpy(), **tol)
            dxb = nhwc_bf16(base) if scatter else ops.new_act(n, cin, h, w, DEV, dtype=torch.bfloat16)
            assert ops._dgrad_b16(dyt, wg, dxb, 2, p, 1, scatter=scatter)
            err = float((dxb.cpu().double() - want).abs().max() / want.abs().max())
            assert err < 2 ** -8, ("bf16 result", err)
        # hooks do not combine with the row maps: nothing is launched, the caller runs the fp32-accurate kernel
        dx = ops.new_act(n, cin, h, w, DEV)
        assert not ops._dgrad_b16(dy16, wg, dx, 2, p, 1, addend=nhwc_bf16(base), scatter=scatter)


@pytest.mark.parametrize("case", [(2, 16, 16, 64, 256), (1, 24, 16, 128, 512), (4, 16, 16, 512, 2048), (2, 32, 32, 64, 128)])
def test_conv_bf16_compute_mode_deferred_batchnorm_backward(ops, case):
    """lin(g, y) in the bf16 loaders (1x1 input gradient and weight gradient; g and y bf16 tensors): the operand is
    bf16(A*g + B*(y - mean) + D) evaluated in fp32 with two fused multiply-adds -- reference: the same expression in fp64 rounded to
    bf16, exact products in fp64; an operand element may round to the neighbouring bf16 value where fp32 and fp64 evaluations differ,
    so the bound is 2^-9 of the result's scale times a small factor (measured ~1e-4), not the 2e-5 of the plain kernels."""
    n, h, w, cin, cout = case
    g = torch.Generator().manual_seed(sum(case) + 3)
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    gq, yq = bf(torch.randn(n, cout, h, w, generator=g)), bf(torch.randn(n, cout, h, w, generator=g))
    lin = torch.stack([0.5 + torch.rand(cout, generator=g), 0.1 * torch.randn(cout, generator=g), 0.2 * torch.randn(cout, generator=g),
                       0.05 * torch.randn(cout, generator=g)])
    v = lambda i: lin[i].double().view(1, -1, 1, 1)
    dy = bf((v(0) * gq.double() + v(1) * (yq.double() - v(2)) + v(3)).float()).double()
    wq = bf(wt).double()
    ref_dx = torch.nn.grad.conv2d_input((n, cin, h, w), wq, dy, 1, 0, 1)
    ref_dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 1, 1), dy, 1, 0, 1)
    ling = lin.to(DEV).contiguous()
    with ops.compute_as(torch.bfloat16):
        dx = ops.new_act(n, cin, h, w, DEV)
        assert ops._dgrad_b16(nhwc_bf16(gq), wl(wt), dx, 1, 0, 1, lin=(nhwc_bf16(yq), ling))
        e = float((dx.cpu().double() - ref_dx).abs().max() / ref_dx.abs().max())
        assert e < 1e-3, e
        dd = ops.DeferredDy(nhwc_bf16(gq), nhwc_bf16(yq), ling, None, None, None)
        dw = torch.empty_like(wl(wt))
        assert ops._wgrad_b16(nhwc_bf16(x), dd, dw, 1, 0, 1, False, None)
        e = float((dw.cpu().double() - ref_dw).abs().max() / ref_dw.abs().max())
        assert e < 1e-3, e


def test_batchnorm_streaming_kernels_eight_channel_form_is_bit_identical(ops, monkeypatch):
    """sh_bn_act and sh_bn_bwd_apply on bf16 tensors move eight channels (one 16-byte access per tensor) per lane in bf16 compute mode;
    the arithmetic per element is the 4-channel form's: outputs, the ReLU quad mask, dy and dres are bit-identical (SEGHIERO_EW8=0
    selects the 4-channel form)."""
    g = torch.Generator().manual_seed(11)
    n, c, h, w = 2, 136, 12, 10
    bf = torch.bfloat16
    y = nhwc_bf16(torch.randn(n, c, h, w, generator=g))
    res = nhwc_bf16(torch.randn(n, c, h, w, generator=g))
    dout = nhwc_bf16(torch.randn(n, c, h, w, generator=g))
    coefs = torch.stack([0.2 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g), torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)]).to(DEV).contiguous()
    gamma = (0.5 + torch.rand(c, generator=g)).to(DEV)
    got = {}
    for form in ("1", "0"):
        monkeypatch.setenv("SEGHIERO_EW8", form)
        out = ops.new_act(n, c, h, w, DEV, dtype=bf)
        mask = ops.new_relu_mask(n, c, h, w, DEV)
        ops.bn_act(y, coefs, out, True, res, mask=mask)
        r = [out.clone(), mask.clone()]
        for relu, o in ((1, out), (2, None), (1, mask), (0, None)):
            dy, dg, db, dres = ops.bn_backward(dout, o, y, coefs, gamma, relu, want_dres=True)
            r += [dy.clone(), dg.clone(), db.clone(), dres.clone()]
        got[form] = r
    for a, b in zip(got["1"], got["0"]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert got["1"][2].dtype == torch.float32           # (outside compute_as: gradients made by bn_backward stay fp32 -- both forms read bf16 y / dout)
    with ops.compute_as(torch.bfloat16):
        for form in ("1", "0"):
            monkeypatch.setenv("SEGHIERO_EW8", form)
            dy, dg, db, dres = ops.bn_backward(dout, mask, y, coefs, gamma, 1, want_dres=True)
            got[form] = [dy.clone(), dres.clone()]
        assert got["1"][0].dtype == bf and torch.equal(got["1"][0], got["0"][0]) and torch.equal(got["1"][1], got["0"][1])
