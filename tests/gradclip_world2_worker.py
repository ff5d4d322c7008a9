"""Child process of tests/test_gpu_gradclip_world2.py: ONE data-parallel rank of the real step (tests/world2_worker.py's set-up:
Trainer(distributed=True) on cuda:0, backend gloo on device tensors) with gradient clipping and the weight EMA on.
    python gradclip_world2_worker.py <rank> <world> <port> <out.pt> <clip_grad_norm> <ema_decay>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

LR = 1e-3


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    clip, decay = float(sys.argv[5]), float(sys.argv[6])
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from test_gpu_train import _no_dropout, build
        from world2_worker import rank_batch
        from mnasnet_pytorch_amd.train_step import Trainer
        torch.manual_seed(100 + rank)                   # ranks start from DIFFERENT parameters: the rank-0 broadcast must fix that
        m = build("512", proj_gamma=0.1).train()
        _no_dropout(m)
        if rank != 0:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01 * torch.randn_like(p))
        tr = Trainer(m, lr=LR, distributed=True, optimizer="sgd", clip_grad_norm=clip, ema_decay=decay)
        assert tr.optimizer.grad_scale == 1.0 / world
        x, t = rank_batch(rank)
        x, t = x.cuda(), t.cuda()
        p0 = tr.flat_p.detach().cpu().clone()           # after the rank-0 broadcast
        e0 = tr.flat_ema.detach().cpu().clone()         # the shadow is taken after it too
        norms, g1, p1 = [], None, None
        for step in range(3):
            tr.step(x, t)
            norms.append(tr.last_grad_norm.clone())     # device tensors: read once at the end
            if step == 0:
                torch.cuda.synchronize()
                g1 = tr.flat_g.detach().cpu().clone()   # the all-reduced (summed) gradient of step 1
                p1 = tr.flat_p.detach().cpu().clone()
        torch.cuda.synchronize()
        torch.save({"flat_p": tr.flat_p.detach().cpu(), "flat_ema": tr.flat_ema.detach().cpu(), "flat_p0": p0, "flat_ema0": e0,
                    "flat_p1": p1, "flat_g1": g1, "norms": torch.cat(norms).cpu(), "stats": tuple(tr.grad_stats()),
                    "world": tr.world}, out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
