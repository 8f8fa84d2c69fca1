"""Times of the image scores on the device (permuto_sdf_amd/image_eval.py) on four 1200 x 1600 x 3 views -- a DTU evaluation
batch -- as uint8 and float32, NCHW and NHWC (an NHWC buffer behind a permuted view, read in place).

Per form and per score: the time between two device events around `repeats` back-to-back calls, divided by the repeats (the calls
read nothing back, so the events bound device work and launch gaps alone), median and spread over `rounds` such windows after a
warm-up; the bytes the pass has to read, computed here from the shapes (both images once; the SSIM pass drops the remainder rows
and columns of the pooling, and its window halo is re-read from cache, not counted), and that count over the median time.  The
count is the algorithm's need, not a counter: GB/s here is "needed bytes over time", not achieved memory traffic.

The comparison is a float32 torch transcription of piq's formula on the same device (avg_pool2d, a grouped conv2d with the
float32 11 x 11 window, the means), fed float32 NCHW images: the only thing a time can be compared with, because no earlier
version of this project computes either score.  It is context, not a threshold: the two do not compute the same thing (float32
against float64 accumulation, LABNOTES.md).  The scores of both are printed so that the comparison is between answers that agree.
One JSON line on stdout; --out writes it to a file as well.

    python tools/image_eval_bench.py --out profiles/image_eval_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import image_eval as ie                    # noqa: E402


def window_ms(fn, repeats):
    """device ms per call over `repeats` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def torch_psnr(x, y):
    return -10 * torch.log10(torch.mean((x - y) ** 2, dim=[1, 2, 3]) + 1e-8)


def torch_ssim(x, y, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    f = max(1, round(min(x.size()[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    coords = torch.arange(kernel_size, dtype=torch.float32, device=x.device) - (kernel_size - 1) / 2.0
    g = coords ** 2
    g = (-(g.unsqueeze(0) + g.unsqueeze(1)) / (2 * sigma ** 2)).exp()
    g /= g.sum()
    C = x.size(1)
    kernel = g.unsqueeze(0).repeat(C, 1, 1, 1)
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = F.conv2d(x, kernel, groups=C), F.conv2d(y, kernel, groups=C)
    sxx = F.conv2d(x * x, kernel, groups=C) - mu_x ** 2
    syy = F.conv2d(y * y, kernel, groups=C) - mu_y ** 2
    sxy = F.conv2d(x * y, kernel, groups=C) - mu_x * mu_y
    ss = (2 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1) * (2 * sxy + c2) / (sxx + syy + c2)
    return ss.mean(dim=(-1, -2)).mean(1)


def views(n, c, h, w, dev):
    """a seeded 8-bit pair: smooth pattern plus noise, uint8 NCHW"""
    g = torch.Generator(device=dev).manual_seed(3)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, 1, h, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, 1, w)
    ch = torch.arange(c, device=dev, dtype=torch.float32).view(1, c, 1, 1)
    gt = (0.5 + 0.4 * torch.sin(xx / (5 + ch)) * torch.cos(yy / 7)).expand(n, c, h, w)
    gt = (gt + 0.02 * torch.randn(n, c, h, w, device=dev, generator=g)).clamp(0, 1)
    pred = (gt + 0.05 * torch.randn(n, c, h, w, device=dev, generator=g)).clamp(0, 1)
    return ie.to_u8(pred), ie.to_u8(gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=50, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_eval_bench measures device times: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    n, c, h, w = args.views, args.channels, args.height, args.width
    pred8, gt8 = views(n, c, h, w, dev)
    mask = (torch.rand(n, 1, h, w, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) > 0.3).to(torch.uint8) * 255
    plan = ie.SsimPlan(n, c, h, w)
    f = plan.factor

    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    forms = {}
    for dtype_name, (p, g_) in (("uint8", (pred8, gt8)), ("float32", (pred8.float() / 255, gt8.float() / 255))):
        forms[dtype_name + "_nchw"] = (p, g_)
        forms[dtype_name + "_nhwc"] = (nhwc(p), nhwc(g_))
    results = {}
    for name, (p, g_) in forms.items():
        el = p.element_size()
        for masked in (False, True):
            m = mask if masked else None
            bytes_psnr = 2 * n * c * h * w * el + (n * h * w if masked else 0)
            bytes_ssim = (2 * n * c * el + (n * c if masked else 0)) * (plan.pooled_h * f) * (plan.pooled_w * f)
            entry = {}
            for score, fn, nbytes in (("psnr", lambda: ie.psnr(p, g_, m, reduction="none"), bytes_psnr),
                                      ("ssim", lambda: ie.ssim(p, g_, m, reduction="none"), bytes_ssim)):
                for _ in range(args.warmup):
                    fn()
                t = spread([window_ms(fn, args.repeats) for _ in range(args.rounds)])
                entry[score] = {"device_ms_per_call": t, "bytes_needed": nbytes,
                                "needed_gb_per_s_at_median": round(nbytes / (t["median"] * 1e-3) / 1e9, 1)}
            entry["psnr_values"] = ie.psnr(p, g_, m, reduction="none").tolist()
            entry["ssim_values"] = ie.ssim(p, g_, m, reduction="none").tolist()
            results[name + ("_masked" if masked else "")] = entry
    xf, yf = forms["float32_nchw"]
    context = {}
    for score, fn in (("psnr", lambda: torch_psnr(xf, yf)), ("ssim", lambda: torch_ssim(xf, yf))):
        for _ in range(args.warmup):
            fn()
        context[score] = {"device_ms_per_call": spread([window_ms(fn, args.repeats) for _ in range(args.rounds)]),
                          "values": fn().double().tolist()}
    result = {"tool": "image_eval_bench", "device": torch.cuda.get_device_name(0), "views": n, "channels": c, "height": h, "width": w,
              "pooling_factor": f, "map": [plan.map_h, plan.map_w], "tiles": [plan.tiles_y, plan.tiles_x],
              "ssim_workgroups": n * c * plan.tiles_y * plan.tiles_x, "sq_diff_workgroups": n * plan.sq_partials,
              "lds_bytes_per_ssim_workgroup": plan.lds_bytes, "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds,
              "forms": results, "torch_float32_piq_formula_context": context}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
