"""Child process of tests/test_gpu_metrics_world2.py: ONE rank of a distributed Trainer.validate on cuda:0 (backend gloo on device
tensors, as tests/world2_worker.py: RCCL refuses two ranks on one device).  Each rank validates its own half of the set; rank 1
starts from perturbed parameters AND perturbed BatchNorm statistics, so only the rank-0 broadcasts (parameters in Trainer, buffers
in validate's sync_buffers) make its half count for the same model.
    python metrics_world2_worker.py <rank> <world> <port> <out.pt>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def val_set(n=4, N=8, classes=10):
    """the whole validation set (closed form: the parent rebuilds it): n batches, two rectangular shapes"""
    import torch
    import cases as C
    out = []
    for i in range(n):
        H, W = (64, 96) if i % 2 == 0 else (96, 64)
        out.append((C.det_input((N, 3, H, W), seed=C.INPUT_SEED + 70 + i), (torch.arange(N) * 3 + i) % classes))
    return out


def build_model():
    import torch
    from test_gpu_train import build
    torch.manual_seed(100)
    m = build("512", proj_gamma=0.1).train()
    with torch.no_grad():                                # running statistics away from (0, 1), the same on every caller
        for k, b in m.named_buffers():
            if k.endswith("running_mean"):
                b.add_(0.05)
            elif k.endswith("running_var"):
                b.mul_(1.25)
    return m


def record(rec):
    return {"steps": rec.steps, "samples": rec.samples, "loss_samples": rec.loss_samples, "correct": dict(rec.correct),
            "last_correct": dict(rec.last_correct), "last_n": rec.last_n, "loss_sum": rec.loss_sum, "loss_avg": rec.loss.avg,
            "loss_val": rec.loss.val, "nonfinite_steps": rec.nonfinite_steps}


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from mnasnet_pytorch_amd.train_step import Trainer
        m = build_model()
        if rank != 0:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01 * torch.randn_like(p))
                for b in m.buffers():
                    if b.dtype.is_floating_point:
                        b.mul_(1.5)
        tr = Trainer(m, lr=1e-3, distributed=True)
        mine = [(x.cuda(), t.cuda()) for i, (x, t) in enumerate(val_set()) if i % world == rank]
        local = record(tr.validate(mine, reduce=False))
        rec = tr.validate(mine)                          # sync_buffers, own half, all_reduce, read
        torch.save({"rank": rank, "world": tr.world, "reduced": record(rec), "local_before_sync": local,
                    "rm0": m.features[0].bn.running_mean.detach().cpu(), "training": m.training}, out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
