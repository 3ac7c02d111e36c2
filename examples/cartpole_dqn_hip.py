"""examples/cartpole_dqn.py with the MLP Q-network on the fused HIP kernels (model.MLP_IMPL =
"hip": act, calc_loss and the update's forward / TD / backward run in rth_mlp_q and
rth_mlp_dqn_grads instead of torch.nn.Linear and autograd).

    python examples/cartpole_dqn_hip.py [max_ts]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cartpole_dqn  # noqa: E402
from reth_amd import model  # noqa: E402


def main(max_ts=cartpole_dqn.MAX_TS, **kwargs):
    prev, model.MLP_IMPL = model.MLP_IMPL, "hip"  # read by DQNSolver at construction
    try:
        worker, trainer, buffer = cartpole_dqn.main(max_ts, **kwargs)
    finally:
        model.MLP_IMPL = prev
    if trainer.solver.mlp_impl_active != "hip":
        raise RuntimeError("the MLP's HIP kernels are not active for this configuration")
    return worker, trainer, buffer


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else cartpole_dqn.MAX_TS)
