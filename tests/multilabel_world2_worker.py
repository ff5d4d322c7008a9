"""Child process of tests/test_gpu_multilabel_world2.py: ONE rank of a distributed multi-label Trainer.validate on cuda:0 (backend
gloo on device tensors, as tests/metrics_world2_worker.py: RCCL refuses two ranks on one device).  Each rank validates its own half
of the set with a MultiClassBCELoss; rank 1 starts from perturbed parameters and BatchNorm statistics, so only the rank-0 broadcasts
make its half count for the same model.
    python multilabel_world2_worker.py <rank> <world> <port> <out.pt>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

INT_FIELDS = ("steps", "samples", "nonfinite_steps", "loss_n", "hdice_n", "f1_n", "tp", "fp", "fn")
SUM_FIELDS = ("loss_sum", "hdice_sum", "f1_sum")


def val_set(n=4, N=8, classes=10):
    """the whole validation set (closed form: the parent rebuilds it): n batches, two rectangular shapes, (N, classes) targets"""
    import torch
    import cases as C
    out = []
    for i in range(n):
        H, W = (64, 96) if i % 2 == 0 else (96, 64)
        t = (((torch.arange(N)[:, None] * 3 + torch.arange(classes)[None, :] + i) % 4) == 0).float()
        out.append((C.det_input((N, 3, H, W), seed=C.INPUT_SEED + 70 + i), t))
    return out


def build_trainer(distributed=False, perturb=False):
    import torch
    from metrics_world2_worker import build_model
    from mnasnet_pytorch_amd import MultiClassBCELoss
    from mnasnet_pytorch_amd.train_step import Trainer
    m = build_model()
    if perturb:
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
            for b in m.buffers():
                if b.dtype.is_floating_point:
                    b.mul_(1.5)
    return m, Trainer(m, lr=1e-3, criterion=MultiClassBCELoss(), distributed=distributed)


def record(rec):
    out = {k: getattr(rec, k) for k in INT_FIELDS + SUM_FIELDS}
    out.update(last_n=rec.last_n, last=(rec.last_tp, rec.last_fp, rec.last_fn),
               last_sums=(rec.last_loss_sum, rec.last_hdice_sum, rec.last_f1_sum),
               val=(rec.loss.val, rec.hdice.val, rec.f1.val), avg=(rec.loss.avg, rec.hdice.avg, rec.f1.avg))
    return out


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        m, tr = build_trainer(distributed=True, perturb=rank != 0)
        mine = [(x.cuda(), t.cuda()) for i, (x, t) in enumerate(val_set()) if i % world == rank]
        local = record(tr.validate(mine, reduce=False))
        from mnasnet_pytorch_amd import MultiLabelMeters
        meters = MultiLabelMeters()
        rec = tr.validate(mine, meters=meters)           # sync_buffers, own half, all_reduce, read
        torch.save({"rank": rank, "world": tr.world, "reduced": record(rec), "local_before_sync": local,
                    "block": meters.block.cpu(), "training": m.training}, out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
