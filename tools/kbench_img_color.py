"""Micro-benchmark of the photometric image ops (mnas_img_color, csrc/mnas_imgc.hip) and of preprocessing type 3 on the device:
us per batch with device events, the bytes each must move, TB/s, and mnas_probe_copy measured in the same process (rate =
2 * bytes / time) so the figure can be read against this box.  N = 256 throughout:
  a  all four jitter ops on every image, CONTRAST last (the mean pass runs the other three too), 512 x 384, NCHW -> NHWC:
     the mean pass and the apply pass (bytes: the input read twice, the output written once)
  b  GRAY in place, 224^2 (bytes: read + written once)
  c  DevicePipeline.from_reference(3) from 640 x 480 sources to 512 x 384 at prob 0.2 and 1.0 (four launches, descriptors
     drawn and uploaded each call: the host side is included), next to type 2 (one launch) measured the same way
Several batches rotate so the inputs do not stay in the 256 MiB Infinity Cache between launches.  One JSON line per workload.
    python tools/kbench_img_color.py [--iters 50]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mnasnet_pytorch_amd import _lib as L                                   # noqa: E402
from mnasnet_pytorch_amd import DevicePipeline, ImageBatch                  # noqa: E402
from mnasnet_pytorch_amd.transforms import color_apply, color_items         # noqa: E402


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


def timed(fn, nsets, iters):
    for i in range(nsets):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % nsets)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_workload(name, lib, n, h, w, desc, il, ol, in_place, read_passes, iters, nsets):
    """mnas_img_color alone: descriptors and workspace already on the device"""
    gen = torch.Generator(device="cuda").manual_seed(0)
    shape = (n, 3, h, w) if il == L.IMGC_NCHW else (n, h, w, 3)
    oshape = (n, 3, h, w) if ol == L.IMGC_NCHW else (n, h, w, 3)
    xs = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
    outs = xs if in_place else [torch.empty(oshape, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    for x, o in zip(xs, outs):
        color_apply(x, desc, il, ol, out=o)                 # checks the descriptors (mnas_img_color_check) and runs once
    items = torch.frombuffer(bytearray(color_items(desc)), dtype=torch.uint8).cuda()
    contrast = any(op == L.IMGC_CONTRAST for d in desc for op, _ in d)
    ws = torch.empty(lib.mnas_img_color_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda") if contrast else None

    def launch(i):
        L.check(lib.mnas_img_color(items.data_ptr(), n, h, w, il, xs[i].data_ptr(), ol, outs[i].data_ptr(), L.ptr(ws),
                                   L.cur_stream()), "mnas_img_color")
    us = timed(launch, nsets, iters)
    nb = n * 3 * h * w
    by = nb * read_passes + nb
    return {"workload": name, "n": n, "size": [h, w], "us_per_batch": round(us, 1), "mbytes": round(by / 1e6, 1),
            "tbs": round(by / (us * 1e-6) / 1e12, 3)}


def pipeline_workload(name, typ, prob, n, iters, nsets):
    """the whole DevicePipeline call per batch, host draws and descriptor uploads included"""
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(nsets):
        imgs = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(n)]
        batches.append(ImageBatch.from_arrays(imgs, target_size=(512, 384)).to("cuda"))
    pipe = DevicePipeline.from_reference(typ, final_size=(512, 384), prob=prob)
    random.seed(0)
    us = timed(lambda i: pipe(batches[i]), nsets, iters)
    return {"workload": name, "n": n, "src": [480, 640], "out": [512, 384], "prob": prob, "us_per_batch": round(us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_img_color needs an MI355X")
    lib = L.load()
    copy0 = probe_copy_tbs(lib)
    random.seed(0)
    n = 256
    jit = []
    for _ in range(n):
        ops = [L.IMGC_BRIGHTNESS, L.IMGC_SATURATION, L.IMGC_HUE]
        random.shuffle(ops)
        jit.append([(op, random.uniform(-0.1, 0.1) if op == L.IMGC_HUE else random.uniform(0.9, 1.1)) for op in ops]
                   + [(L.IMGC_CONTRAST, random.uniform(0.9, 1.1))])
    rows = [kernel_workload("a_jitter4_contrast_last_512x384_nchw_to_nhwc", lib, n, 512, 384, jit, L.IMGC_NCHW, L.IMGC_NHWC,
                            False, 2, a.iters, a.sets),
            kernel_workload("b_gray_in_place_224", lib, n, 224, 224, [[(L.IMGC_GRAY, 0.0)]] * n, L.IMGC_NCHW, L.IMGC_NCHW,
                            True, 1, a.iters, a.sets)]
    copy1 = probe_copy_tbs(lib)
    copy = (copy0 + copy1) / 2
    for r in rows:
        r["probe_copy_tbs"] = round(copy, 3)
        r["of_copy"] = round(r["tbs"] / copy, 3)
    iters_c = max(5, a.iters // 5)
    rows += [pipeline_workload("c_type3_prob0.2_512x384", 3, 0.2, n, iters_c, a.sets),
             pipeline_workload("c_type3_prob1.0_512x384", 3, 1.0, n, iters_c, a.sets),
             pipeline_workload("c_type2_512x384", 2, 0.2, n, iters_c, a.sets)]
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
