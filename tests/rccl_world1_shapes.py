"""Child process of tests/test_gpu_shard_shapes.py: an RCCL ("nccl") process group of ONE rank on cuda:0, created before any
other GPU call of the process; libspectral's own communicator (native_comm_init) then drives the streaming engine
(NativeWelchPipeline: export, all-reduce, apply) at shapes of the generic one-pass kernel, five steps with different data each.
Prints one JSON line."""
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)      # first GPU call of the process
    torch.cuda.set_device(0)
    from pyfft_amd import engine as E
    from pyfft_amd.dist import shard_plan, welch_psd_sharded, native_comm_init, NativeWelchPipeline
    from oracle import cpu_ref as O

    out = {"backend": dist.get_backend(), "native_comm": list(native_comm_init(device=0)), "steps": []}
    worst, worst_o = 0.0, 0.0
    gen = torch.Generator(device="cuda").manual_seed(11)
    for nfft, hop, cplx in ((4096, 1351, True), (2981, 992, False)):
        total = nfft + hop * 2000 + 77
        plan = shard_plan(total, nfft, hop, 1, 0)
        win = O.windows("Blackman-Harris", nwins=nfft)
        xs = []
        for k in range(5):
            if cplx:
                z = torch.randn(total, 2, device=dev, generator=gen) + torch.tensor([0.4 * k, 0.1 - 0.2 * k], device=dev)
                xs.append(torch.view_as_complex(z.contiguous()))
            else:
                xs.append(torch.randn(total, device=dev, generator=gen) * (1.0 + 0.5 * k) - 1.5 * k)
        pipe = NativeWelchPipeline(win, plan, scale=1.0, sided=E.SIDED_TWO)
        got = [r for r in (pipe.submit(x) for x in xs) if r is not None] + pipe.flush_all()
        out["steps"].append(len(got))
        for x, g in zip(xs, got):
            one = welch_psd_sharded(x, win, plan, scale=1.0, sided=E.SIDED_TWO)
            worst = max(worst, float(torch.max(torch.abs(g - one) / (1e-6 * torch.abs(one) + 1e-9 * one.max())).item()))
        xh = xs[0].cpu().numpy().astype(np.complex128 if cplx else np.float64)
        ref = torch.from_numpy(O.welch_psd_stream(xh, win, nfft, hop, plan.frames_total, 1.0) * np.sum(win ** 2))
        g0 = got[0].cpu()
        worst_o = max(worst_o, float(torch.max(torch.abs(g0 - ref) / (2e-4 * torch.abs(ref) + 1e-6 * ref.max())).item()))
    out["vs_sharded"] = worst
    out["vs_oracle"] = worst_o
    torch.cuda.synchronize()
    E.comm_destroy()
    dist.destroy_process_group()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
