"""Micro-benchmark of the image batch transform (mnas_img_xform, csrc/mnas_imgx.hip): us per batch with device events, the
bytes it must move (the source crops read + the NCHW uint8 output written), TB/s, and mnas_probe_copy measured in the same
process (rate = 2 * bytes / time) so the figure can be read against this box.  Two workloads, both N = 256:
  w1  500 x 375 sources, reference type 4 (RandomResizedCropRect + RandomHorizontalFlip) -> 224^2
  w2  640 x 480 sources, reference type 2 (Resize(final_size)) -> 512 x 384
Several batches rotate so the sources do not stay in the 256 MiB Infinity Cache between launches.  One JSON line per workload.
    python tools/kbench_img_xform.py [--iters 50]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mnasnet_pytorch_amd import _lib as L                       # noqa: E402
from mnasnet_pytorch_amd import DeviceTransform, ImageBatch     # noqa: E402
from mnasnet_pytorch_amd.transforms import apply                # noqa: E402


def probe_copy_tbs(lib, nbytes=1 << 30, iters=20):
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        L.check(lib.mnas_probe_copy(a.data_ptr(), b.data_ptr(), nbytes, L.cur_stream()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.check(lib.mnas_probe_copy(a.data_ptr(), b.data_ptr(), nbytes, L.cur_stream()))
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * iters / (e0.elapsed_time(e1) * 1e-3) / 1e12


def workload(name, h, w, tf, size, n, iters, nsets):
    rng = np.random.default_rng(0)
    random.seed(0)
    lib = L.load()
    sets = []
    for _ in range(nsets):
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
        batch = ImageBatch.from_arrays(imgs).to("cuda")
        hw, desc = tf.describe(batch.shapes, size)
        want = apply(batch, desc, hw)                   # checks the descriptors (mnas_img_xform_check) and runs once
        items = torch.frombuffer(bytearray(DeviceTransform.descriptors(batch, desc)), dtype=torch.uint8).cuda()
        sets.append((batch, items, hw, desc, torch.empty_like(want)))
    hw = sets[0][2]
    # algorithmic bytes: every crop read once, every output byte written once
    rd = sum(d[2] * d[3] * 3 for s in sets for d in s[3]) / nsets
    wr = n * 3 * hw[0] * hw[1]

    def launch(s):          # the kernel alone: descriptors already on the device
        batch, items, _, _, out = s
        L.check(lib.mnas_img_xform(items.data_ptr(), n, hw[0], hw[1], batch.data.data_ptr(), batch.data.numel(), out.data_ptr(),
                                   L.cur_stream()), "mnas_img_xform")
    for s in sets:
        launch(s)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        launch(sets[i % nsets])
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    return {"workload": name, "n": n, "src": [h, w], "out": list(hw), "us_per_batch": round(us, 1),
            "mbytes": round((rd + wr) / 1e6, 1), "mbytes_read": round(rd / 1e6, 1), "mbytes_written": round(wr / 1e6, 1),
            "tbs": round((rd + wr) / (us * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_img_xform needs an MI355X")
    lib = L.load()
    copy0 = probe_copy_tbs(lib)
    rows = [workload("w1_type4_224", 375, 500, DeviceTransform.from_reference(4, final_size=(224, 224)), None, 256, a.iters, a.sets),
            workload("w2_type2_512x384", 480, 640, DeviceTransform.from_reference(2, final_size=(512, 384)), None, 256, a.iters,
                     a.sets)]
    copy1 = probe_copy_tbs(lib)
    copy = (copy0 + copy1) / 2
    for r in rows:
        r["probe_copy_tbs"] = round(copy, 3)
        r["of_copy"] = round(r["tbs"] / copy, 3)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
