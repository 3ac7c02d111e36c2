"""Microbench (development aid): FC1's backward (gy [B, 512], x [B, 3136], w [512, 3136] ->
gx = gy w, gw = gy^T x) on hipBLASLt (the two torch.mm calls of the learner, the committed
TunableOp picks) vs rth_fc_bwd (both gradients in one call), alone, HIP events, three rounds
interleaved.  FCB_BS=64,512 picks the batch sizes."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reth_amd import _lib, gemm_tuning  # noqa: E402

dev = torch.device("cuda")
gemm_tuning.enable()
N, K = 512, 3136
for B in [int(v) for v in os.environ.get("FCB_BS", "64,512").split(",")]:
    gy = (torch.rand((B, N), device=dev) * 2 - 1) * (torch.rand((B, N), device=dev) < 0.5)
    x = torch.rand((B, K), device=dev) * 3 / B ** 0.5
    w = (torch.rand((N, K), device=dev) * 2 - 1) / N ** 0.5
    gx, gw = torch.empty((B, K), device=dev), torch.empty((N, K), device=dev)

    def library():
        torch.mm(gy, w, out=gx)
        torch.mm(gy.t(), x, out=gw)

    fns = {"hipblaslt 2 x mm": library}
    if _lib.lib().rth_fc_bwd_supported(B, N, K):
        ws = torch.empty(max(_lib.lib().rth_fc_bwd_workspace(B, N, K), 16) // 4, device=dev)
        fns["rth_fc_bwd"] = lambda: _lib.call("rth_fc_bwd", gy.data_ptr(), N, x.data_ptr(), K, w.data_ptr(), B, N, K,
                                              gx.data_ptr(), gw.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    rx, rw = gy.double() @ w.double(), gy.double().t() @ x.double()
    res = {name: [] for name in fns}
    err = {}
    for name, fn in fns.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        err[name] = max(float((gx.double() - rx).abs().max()), float((gw.double() - rw).abs().max()))
    for _ in range(3):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / 200)
    fl = 4.0 * B * N * K
    print(f"B={B}: " + "  ".join(f"{k} {' / '.join(f'{t:.1f}' for t in v)} us ({fl / min(v) / 1e6:5.1f} TF/s, "
                                 f"err {err[k]:.1e})" for k, v in res.items()), flush=True)
