"""rth_conv_wgrad_f32's cross-wave sum (r15: every wave stores its accumulator block, every
thread adds and stores its share) on inputs whose sums are exact in any order: small integers
scaled by a power of two, so every product and every partial sum is an integer multiple of 2^-5
far below 2^24 of them -- the result must equal the integer result computed on the CPU exactly.
This pins that every term is there exactly once; that the order is r06's follows from the code
(profiles/r15/bits.txt holds the digests of seeded random inputs under both epilogues)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMS = {"conv2": (32, 20, 20, 64, 4, 2), "conv3": (64, 9, 9, 64, 3, 1)}


# n: 1 = most waves of most workgroups get an empty pair range; 3 = an odd pixel count, the last
# pair half past the batch; 64 = every wave busy
@pytest.mark.parametrize("n", [1, 3, 64])
@pytest.mark.parametrize("geom", ["conv2", "conv3"])
def test_conv_wgrad_f32_exact_integers(dev, geom, n):
    from reth_amd import _lib

    cin, h, wd, cout, k, s = GEOMS[geom]
    ho = (h - k) // s + 1
    assert (n * ho * ho) % 2 == n % 2  # both geometries: an odd pixel count per sample
    gen = torch.Generator().manual_seed(7 * n + cin)
    x = torch.randint(-3, 4, (n, cin, h, wd), generator=gen).double() / 4
    gy = torch.randint(-3, 4, (n, cout, ho, ho), generator=gen).double() / 8
    assert n * ho * ho * 9 < 2 ** 24  # |sum| * 32 stays an exact fp32 integer
    w = torch.zeros((cout, cin, k, k), dtype=torch.float64)
    _, want, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                                     [False, True, False])
    assert torch.equal(want * 32, (want * 32).round())
    shape = _lib.ConvShape(_lib.CONV_F32_NHWC, cin, h, wd, cout, k, k, s)
    ws = torch.empty(_lib.lib().rth_conv_wgrad_f32_workspace(_lib.ctypes.byref(shape)) // 4, device=dev)
    xd = x.float().to(dev).contiguous(memory_format=torch.channels_last)
    gyd = gy.float().to(dev).contiguous(memory_format=torch.channels_last)
    gw = torch.full((cout, cin, k, k), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    _lib.call("rth_conv_wgrad_f32", _lib.ctypes.byref(shape), xd.data_ptr(), n, gyd.data_ptr(), gw.data_ptr(),
              ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), want)
