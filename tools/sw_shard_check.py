"""Run under torch.distributed.run with 2 ranks on ONE GPU over gloo (tests/test_gpu_baseline.py):
sliding-window inference with shard_ranks=True must return, on every rank, exactly what a single rank computes; the
default mode must leave every rank alone with its own volume (no collective)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from medicalsemseg_amd import parallel  # noqa: E402
from medicalsemseg_amd.engine.utils import sliding_window_inference  # noqa: E402
from medicalsemseg_amd.models.unet import UNET_FEATURES, UNet  # noqa: E402


def main():
    parallel.init_from_env()
    rk, ws = parallel.rank(), parallel.world_size()
    assert ws == 2
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = UNet(1, 2, UNET_FEATURES["UNetSmall"], compute_dtype=torch.bfloat16).to(dev).eval()
    aff = torch.ones(1, 3, device=dev)
    g = torch.Generator().manual_seed(11)
    shared = torch.randn(1, 1, 48, 64, 80, generator=g).to(dev)

    class Plain(torch.nn.Module):     # a predictor without graph_safe / infer_cl: the generic path
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x_in):
            return self.inner(x_in)

    with torch.no_grad():
        for pred, tag in ((net, "graphed"), (Plain(net), "generic")):
            for roi, nb in (((32, 32, 32), 2), ((32, 32, 32), 3), ((48, 64, 80), 2)):   # last: ONE window < 2 ranks
                single = sliding_window_inference(shared, aff, roi, nb, pred, overlap=0.5, mode="gaussian")
                sharded = sliding_window_inference(shared, aff, roi, nb, pred, overlap=0.5, mode="gaussian",
                                                   shard_ranks=True)
                assert torch.equal(single, sharded), (tag, roi, nb, rk, float((single - sharded).abs().max()))
            # mirror test-time augmentation: 8 rows per window, 3 per batch -> steps straddle windows and ranks
            kw = dict(overlap=0.5, mode="gaussian", mirror_axes=(0, 1, 2))
            single = sliding_window_inference(shared, aff, (32, 32, 32), 3, pred, **kw)
            sharded = sliding_window_inference(shared, aff, (32, 32, 32), 3, pred, shard_ranks=True, **kw)
            assert torch.equal(single, sharded), (tag, "mirror", rk, float((single - sharded).abs().max()))
        # default mode: each rank its own volume, result == what the same call gives without a process group view
        mine = torch.randn(1, 1, 48, 48, 48, generator=torch.Generator().manual_seed(100 + rk)).to(dev)
        a = sliding_window_inference(mine, aff, (32, 32, 32), 2, net, overlap=0.5, mode="gaussian")
        ws_fn = parallel.world_size
        parallel.world_size = lambda: 1          # what a single process would compute
        try:
            b = sliding_window_inference(mine, aff, (32, 32, 32), 2, net, overlap=0.5, mode="gaussian")
        finally:
            parallel.world_size = ws_fn
        assert torch.equal(a, b)
    torch.distributed.barrier()
    if rk == 0:
        print("SHARD_CHECK_OK", flush=True)
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
