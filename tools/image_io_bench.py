"""Times the image I/O calls (where2edit_amd/image_io.py, csrc/image.hip) against what a user would otherwise run, and the captured
config-5 pipeline with bytes at both ends against floats at both ends.

  to_tensor   uint8 [B,1024,1024,3] -> fp32 [B,3,256,256]   vs  permute -> float -> F.interpolate(bilinear, antialias) -> / 255 -> normalise
  label_ids   uint8 [B,512,512]     -> uint8 [B,64,64]      vs  float -> F.interpolate(bilinear, antialias) -> round -> uint8
              (the stock pixels are close to Pillow's, not equal: the largest distance in grey levels / the share of differing ids is
              reported, not asserted)
              and, where PIL imports, Pillow's own resize (+ the numpy ToTensor / Normalize) on one host core
  to_bytes    fp32 [B,3,1024,1024]  -> uint8 [B,1024,1024,3] (grid=False) and the make_grid canvas (grid=True)
                                                            vs  the op sequence of torchvision 0.8.2's save_image on the device
  pipeline    capture_invert_and_edit at batch 8, float in / float out against uint8 in / uint8 out, each with the device-to-host
              copy of its images and mask into pinned memory

  --jpeg      to_jpeg  uint8 [B,1024,1024,3] -> B files     vs  .cpu(), then Pillow's save per image on one host core
              save_image  fp32 [B,3,1024,1024] -> one file  vs  to_bytes, .cpu(), Pillow's save   (B = 1, 4, 8: a row of B images;
                                                                and B = 8 with nrow = 4: the 2 x 4 grid canvas)
              both ends on the host, so these are host-clock times of whole calls (time_host); and the two stages of the encoder
              alone (w2e_jpeg_coefficients, w2e_jpeg_entropy) on device events, with the bytes each moves.  Smooth-plus-noise
              images, not noise.  Lines go to --jpeg-out (profiles/jpeg_bench.jsonl).

  --decode    from_jpeg  B files -> uint8 [B,1024,1024,3]   vs  Pillow's decoder per file on one host core, then .to("cuda")
              (the photograph of tests/jpeg_ref.py at quality 75 and 95, B = 1 and 8, sub_bits 256 / 512 / 1024; the constant image:
              the relaxation's worst case) on the host clock, with the number of launches; and the stages alone.  Lines go to
              --decode-out (profiles/jpeg_decode_bench.jsonl).

  --png       from_png  B files -> uint8 pixels             vs  Pillow's decoder per file on one host core, then .to("cuda")
              (B = 1, 8, 90 label-like 512 x 512 grey files of a few dozen flat regions, mode="raw"; one noisy 1024 x 1024 RGB file
              and B = 8 of them, mode="RGB"; the files are written here, with zlib) on the host clock, and the two stages alone
              (w2e_png_inflate, w2e_png_pixels) on device events.  Lines go to --png-out (profiles/png_decode_bench.jsonl).

  --png-encode  to_png  uint8 [B,H,W,C] -> B files          vs  .cpu(), then Pillow's PNG save per image on one host core
              (B = 1 and 8 photo-like 1024 x 1024 RGB canvases; B = 1 and 90 label-like 512 x 512 grey images; B = 8 noise canvases,
              the worst case: every chunk stored, and the second copy) on the host clock, with the bytes of the files of both; and the
              two stages alone (w2e_png_filter, w2e_png_deflate) on device events.  Lines go to --png-encode-out
              (profiles/png_encode_bench.jsonl).

HIP events around `--inner` back-to-back calls of the Python entry point, device-synchronised, after a warm-up; the variants of a
group alternate, `--repeats` times each (>= 5): the median, with min .. max as the spread a difference has to exceed.  `bytes` is
what the call has to move (input + output), GB/s = bytes / median.  One JSON line per (group, variant, batch), appended to --out.

    python tools/image_io_bench.py [--repeats 20] [--inner 10] [--skip-pipeline] [--out profiles/image_io_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stock_to_tensor(x, size, mean=0.5, std=0.5):
    y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size, mode="bilinear", antialias=True, align_corners=False)
    return y.div(255).sub_(mean).div_(std)


def stock_label_ids(x, size):
    y = F.interpolate(x[:, None].float(), size=size, mode="bilinear", antialias=True, align_corners=False)
    return y.round_().clamp_(0, 255).to(torch.uint8)[:, 0]


def stock_to_bytes(x, lo=-1.0, hi=1.0, nrow=8, padding=2, grid=True):
    """torchvision 0.8.2 utils.save_image up to the byte tensor, on the device the images are on."""
    t = x.clone()
    t.clamp_(min=lo, max=hi)
    t.add_(-lo).div_(hi - lo + 1e-5)
    if not grid:
        return t.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()
    b, _, h, w = t.shape
    if b == 1:
        canvas = t[0]
    else:
        xmaps = min(nrow, b)
        ymaps = -(-b // xmaps)
        canvas = t.new_full((3, (h + padding) * ymaps + padding, (w + padding) * xmaps + padding), 0.0)
        for k in range(b):
            yy, xx = divmod(k, xmaps)
            canvas.narrow(1, yy * (h + padding) + padding, h).narrow(2, xx * (w + padding) + padding, w).copy_(t[k])
    return canvas.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def time_group(variants, repeats, inner):
    """{name: [ms per call]}: the variants alternate; an interval is `inner` calls between two events."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    return times


def line(group, variant, batch, ms, nbytes, **extra):
    med = statistics.median(ms)
    out = {"tool": "image_io_bench", "group": group, "variant": variant, "batch": batch, "bytes": nbytes, "ms_median": med, "ms_min": min(ms),
           "ms_max": max(ms), "repeats": len(ms), "gb_per_s": nbytes / med / 1e6}
    out.update(extra)
    return out


def pillow_ms(x_host, size, label, repeats=5):
    """Median ms per IMAGE of Pillow's resize (+ ToTensor / Normalize in numpy for images) on this process' one thread, or None."""
    try:
        import numpy as np
        from PIL import Image
    except ImportError:
        return None
    img = Image.fromarray(x_host[0].numpy(), "L" if label else "RGB")
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = np.asarray(img.resize((size, size), getattr(Image, "Resampling", Image).BILINEAR))
        if not label:
            r = (r.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def bench_calls(a, lines):
    from where2edit_amd import image_io as I
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    for b in (1, 8):
        img = torch.randint(0, 256, (b, 1024, 1024, 3), generator=g, dtype=torch.uint8)
        lab = torch.randint(0, 19, (b, 16, 16), generator=g, dtype=torch.uint8).repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
        img_d, lab_d = img.to(dev), lab.to(dev)
        ours, stock = I.to_tensor(img_d, 256), stock_to_tensor(img_d, (256, 256))
        differ_img = float((ours - stock).abs().max()) * 127.5  # in grey levels: Normalize(0.5, 0.5) maps one level to 1 / 127.5
        differ_lab = float((I.label_ids(lab_d, 64) != stock_label_ids(lab_d, (64, 64))).float().mean())
        nb_img, nb_lab = img.numel() + b * 3 * 256 * 256 * 4, lab.numel() + b * 64 * 64
        t = time_group({"hip": lambda: I.to_tensor(img_d, 256), "stock": lambda: stock_to_tensor(img_d, (256, 256))}, a.repeats, a.inner)
        lines.append(line("to_tensor_1024_256", "hip", b, t["hip"], nb_img))
        lines.append(line("to_tensor_1024_256", "stock", b, t["stock"], nb_img, max_grey_levels_from_hip=differ_img))
        t = time_group({"hip": lambda: I.label_ids(lab_d, 64), "stock": lambda: stock_label_ids(lab_d, (64, 64))}, a.repeats, a.inner)
        lines.append(line("label_ids_512_64", "hip", b, t["hip"], nb_lab))
        lines.append(line("label_ids_512_64", "stock", b, t["stock"], nb_lab, values_differing_from_hip=differ_lab))
        if b == 1:
            for group, x, size, label, nbytes in (("to_tensor_1024_256", img, 256, False, nb_img), ("label_ids_512_64", lab, 64, True, nb_lab)):
                ms = pillow_ms(x, size, label)
                if ms is not None:
                    lines.append(line(group, "pillow_one_host_core_per_image", 1, [ms], nbytes))
        x = (torch.rand(b, 3, 1024, 1024, generator=g) * 2.2 - 1.1).to(dev)
        for grid in (False, True):
            ours, stock = I.to_bytes(x, grid=grid), stock_to_bytes(x, grid=grid)
            differ = float((ours != stock).float().mean()) if ours.shape == stock.shape else 1.0
            nb = x.numel() * 4 + ours.numel()
            t = time_group({"hip": lambda: I.to_bytes(x, grid=grid), "stock": lambda: stock_to_bytes(x, grid=grid)}, a.repeats, a.inner)
            group = "to_bytes_1024_grid" if grid else "to_bytes_1024"
            lines.append(line(group, "hip", b, t["hip"], nb))
            lines.append(line(group, "stock", b, t["stock"], nb, values_differing_from_hip=differ))
        del x, img_d, lab_d


def bench_pipeline(a, lines, batch=8):
    import bench  # build_config5: the modules and inputs of the config-5 benchmark
    from where2edit_amd.demo_pipeline import capture_invert_and_edit
    dev = torch.device("cuda")
    imgs, e4e, g, clip, net, text, att = bench.build_config5(dev, batch, 0)
    gen = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (batch, 1024, 1024, 3), generator=gen, dtype=torch.uint8).to(dev)
    run_f = capture_invert_and_edit(imgs, e4e, g, clip, net, text, att, attention_layer=13)
    run_b = capture_invert_and_edit(u8, e4e, g, clip, net, text, att, attention_layer=13, as_bytes=True)
    keys_f, keys_b = ("img_orig", "img_gen", "mask"), ("img_orig_u8", "img_gen_u8", "mask_u8")
    out_f, out_b = run_f(imgs, text, att), run_b(u8, text, att)
    pinned = {k: torch.empty(out.shape, dtype=out.dtype, pin_memory=True) for o, keys in ((out_f, keys_f), (out_b, keys_b)) for k, out in
              ((k, o[k]) for k in keys)}

    def step(run, x, keys):
        out = run(x, text, att)
        for k in keys:
            pinned[k].copy_(out[k], non_blocking=True)

    t = time_group({"float_in_float_out": lambda: step(run_f, imgs, keys_f), "uint8_in_uint8_out": lambda: step(run_b, u8, keys_b)}, a.repeats, 1)
    for name, x, keys in (("float_in_float_out", imgs, keys_f), ("uint8_in_uint8_out", u8, keys_b)):
        d2h = sum(pinned[k].numel() * pinned[k].element_size() for k in keys)
        med = statistics.median(t[name])
        lines.append(line("config5_captured_with_d2h", name, batch, t[name], d2h, images_per_s=batch / med * 1e3, input_bytes=x.numel() * x.element_size(),
                          d2h_bytes=d2h))


def time_host(variants, repeats):
    """{name: [ms per call]} on the host clock: every variant ends with its bytes on the host, so the call itself synchronises.  The
    variants alternate; the device is drained before each interval."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {n: [] for n in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def photo_u8(b, h, w, seed):
    """Smooth plus noise, uint8 [b,h,w,3]: the statistics of a generated face more than those of noise (which no JPEG compresses)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h) / h, torch.arange(w) / w, indexing="ij")
    base = torch.stack([128 + 100 * torch.sin(6 * xx + 2 * yy), 128 + 100 * torch.cos(5 * yy - xx), 128 + 90 * torch.sin(9 * xx * yy)], -1)
    return (base[None] + 6 * torch.randn(b, h, w, 3, generator=g)).clamp_(0, 255).to(torch.uint8)


def bench_jpeg(a, lines):
    """to_jpeg / save_image against what a caller does today (the canvas to the host, Pillow's encoder on one host core), and the two
    stages of the encoder alone.  Host-clock times for the calls that end on the host, device events for the stages."""
    import io
    from where2edit_amd import image_io as I
    from where2edit_amd._lib import call, stream_ptr
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = "cuda"

    def pillow(canvas_host):
        buf = io.BytesIO()
        Image.fromarray(canvas_host.numpy()).save(buf, format="JPEG")
        return buf.getvalue()

    for b in (1, 4, 8):
        u8 = photo_u8(b, 1024, 1024, b).to(dev)
        files = I.to_jpeg(u8)
        coded = sum(len(f) for f in files)
        variants = {"hip": lambda: I.to_jpeg(u8)}
        extra = {"coded_bytes": coded}
        if Image is not None:
            variants["d2h_then_pillow"] = lambda: [pillow(img) for img in u8.cpu()]
            extra["equal_to_pillow"] = files == [pillow(img) for img in u8.cpu()]
        t = time_host(variants, a.repeats)
        for name, ms in t.items():
            lines.append(line("to_jpeg_1024", name, b, ms, u8.numel() + coded, **extra))
        # the stages alone
        plan = I.jpeg_plan(b, 1024, 1024)
        coef = torch.empty((b, plan["blocks"], 64), dtype=torch.int16, device=dev)
        out = torch.empty((b, plan["segment"]), dtype=torch.uint8, device=dev)
        lengths = torch.empty((b,), dtype=torch.int64, device=dev)
        work = torch.empty((plan["workspace"],), dtype=torch.uint8, device=dev)
        huff = I._huff_table(torch.device(dev, torch.cuda.current_device()))
        stage1 = lambda: call("w2e_jpeg_coefficients", I._p(u8), b, 1024, 1024, 75, I._p(coef), stream_ptr())
        stage2 = lambda: call("w2e_jpeg_entropy", I._p(coef), b, 1024, 1024, I._p(huff), I._p(out), plan["segment"], I._p(lengths), I._p(work), stream_ptr())
        stage1()
        t = time_group({"coefficients": stage1, "entropy": stage2}, a.repeats, a.inner)
        seg = int(lengths.sum())
        lines.append(line("jpeg_stage_1024", "coefficients", b, t["coefficients"], u8.numel() + coef.numel() * 2))
        # entropy: coefficients in, slot words and lengths out and in again, offsets out and in, the segment out
        lines.append(line("jpeg_stage_1024", "entropy", b, t["entropy"], coef.numel() * 2 + 2 * (seg + 4 * b * plan["blocks"]) + 16 * b * plan["blocks"] + seg,
                          segment_bytes=seg))
        del coef, out, work
        x = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
        for nrow, group in ((8, "save_image_1024"),) + (((4, "save_image_1024_grid_2x4"),) if b == 8 else ()):
            def ours():
                buf = io.BytesIO()
                I.save_image(x, buf, nrow=nrow)
                return buf.getvalue()
            variants = {"hip": ours}
            extra = {"coded_bytes": len(ours()), "canvas": list(I.grid_shape(b, 1024, 1024, nrow))}
            if Image is not None:
                variants["to_bytes_d2h_then_pillow"] = lambda: pillow(I.to_bytes(x, nrow=nrow).cpu())
                extra["equal_to_pillow"] = ours() == variants["to_bytes_d2h_then_pillow"]()
            t = time_host(variants, a.repeats)
            for name, ms in t.items():
                lines.append(line(group, name, b, ms, x.numel() * 4 + extra["coded_bytes"], **extra))
        del x, u8


def bench_decode(a, lines):
    """from_jpeg against what a caller does today (Pillow's decoder on one host core, then the pixels to the device), for the
    1024 x 1024 photograph of tests/jpeg_ref.py at quality 75 and 95, batches of 1 and 8, subsequences of 256 / 512 / 1024 bits; the
    constant image, whose relaxation takes as many rounds as it has subsequences; and the stages alone.  Host-clock times of whole
    calls (both end synchronised), device events for the stages that do not synchronise."""
    import io
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_ref as R
    from where2edit_amd import image_io as I
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda", torch.cuda.current_device())
    subs = (256, 512, 1024)

    def pillow(files):
        out = torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])).to(dev)
        torch.cuda.synchronize()
        return out

    for quality in (75, 95):
        for b in (1, 8):
            files = I.to_jpeg(torch.from_numpy(np.stack([R.photo(1024, 1024, seed) for seed in range(b)])).to(dev), quality)
            coded = sum(len(f) for f in files)
            variants = {f"hip_sub{sb}": (lambda sb=sb: I.from_jpeg(files, sub_bits=sb, stack=True)) for sb in subs}
            extra = {"quality": quality, "coded_bytes": coded}
            if Image is not None:
                variants["pillow_then_h2d"] = lambda: pillow(files)
                extra["equal_to_pillow"] = all(torch.equal(fn(), pillow(files)) for name, fn in variants.items() if name.startswith("hip"))
            t = time_host(variants, a.repeats)
            for name, ms in t.items():
                launches = I.jpeg_decode_states(files, int(name[7:]))[1] if name.startswith("hip") else None
                lines.append(line("from_jpeg_1024", name, b, ms, coded + b * 1024 * 1024 * 3, launches=launches, **extra))
            # the stages alone
            parsed = [I.jpeg_parse(f) for f in files]
            for sb in subs:
                batch = I._JpegBatch(parsed, dev, sb)
                t = time_host({"relax": batch.relax}, a.repeats)
                lines.append(line("jpeg_decode_stage_1024", f"relax_sub{sb}", b, t["relax"], coded, launches=batch.relax(), quality=quality,
                                  subsequences=batch.plan["subsequences"]))
                coef, status = batch.coefficients()
                quant = batch.quant.to(dev)
                t = time_group({"coefficients": batch.coefficients, "pixels": lambda: I._jpeg_pixels(coef, quant, 1024, 1024, batch.sampling, batch.plan)},
                               a.repeats, a.inner)
                lines.append(line("jpeg_decode_stage_1024", f"coefficients_sub{sb}", b, t["coefficients"], 2 * coded + coef.numel() * 2, quality=quality))
                if sb == subs[-1]:
                    lines.append(line("jpeg_decode_stage_1024", "pixels", b, t["pixels"], coef.numel() * 2 + 2 * b * 1024 * 1024 * 3 // 2 + b * 1024 * 1024 * 3,
                                      quality=quality))
                del batch, coef
    # the worst case of the relaxation: every MCU of a constant image codes alike, so a wrong phase never meets the right one
    flat = I.to_jpeg(torch.from_numpy(R.pattern("constant", 1024, 1024)).to(dev))
    variants = {f"hip_sub{sb}": (lambda sb=sb: I.from_jpeg(flat, sub_bits=sb)) for sb in subs}
    if Image is not None:
        variants["pillow_then_h2d"] = lambda: pillow([flat])
    t = time_host(variants, a.repeats)
    for name, ms in t.items():
        states, launches = I.jpeg_decode_states(flat, int(name[7:])) if name.startswith("hip") else (None, None)
        lines.append(line("from_jpeg_1024_constant", name, 1, ms, len(flat) + 1024 * 1024 * 3, launches=launches, coded_bytes=len(flat),
                          subsequences=None if states is None else int(states.shape[0])))


def bench_png(a, lines):
    """from_png against what a caller does today (Pillow's decoder on one host core, then the pixels to the device): batches of
    label-like 512 x 512 grey files and noisy 1024 x 1024 RGB files, written by tests/png_ref.py's writer (zlib level 6; the labels
    unfiltered, the photographs with the Paeth filter).  Host-clock times of whole calls (both end synchronised); the two stages on
    device events, one pair per repeat (stage 2 keeps rows in stage 1's output, so the pair runs together)."""
    import io
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import png_ref as P
    from where2edit_amd import image_io as I
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda", torch.cuda.current_device())

    def label(seed):  # a few dozen flat regions: rectangles of ids 0..18 over one another
        rng = np.random.default_rng(seed)
        x = np.zeros((512, 512), np.uint8)
        for _ in range(40):
            y0, x0 = rng.integers(0, 448, 2)
            x[y0:y0 + rng.integers(16, 200), x0:x0 + rng.integers(16, 200)] = rng.integers(0, 19)
        return x

    def pillow(files, mode):
        images = [Image.open(io.BytesIO(f)) for f in files]
        out = torch.from_numpy(np.stack([np.asarray(im.convert("RGB") if mode == "RGB" else im) for im in images])).to(dev)
        torch.cuda.synchronize()
        return out

    def ours(files, mode):
        out = I.from_png(files, mode=mode, stack=True)
        torch.cuda.synchronize()
        return out

    cases = [("from_png_label_512", "raw", 0, [P.write_png(label(i), 0, filters=0, level=6) for i in range(90)], (1, 8, 90)),
             ("from_png_rgb_1024", "RGB", 2, [P.write_png(photo_u8(1, 1024, 1024, i)[0].numpy(), 2, filters=4, level=6) for i in range(8)], (1, 8))]
    for group, mode, colour, files, batches in cases:
        for b in batches:
            fs = files[:b]
            coded = sum(len(f) for f in fs)
            want = ours(fs, mode)
            variants = {"hip": lambda: ours(fs, mode)}
            extra = {"coded_bytes": coded, "mode": mode}
            if Image is not None:
                variants["pillow_then_h2d"] = lambda: pillow(fs, mode)
                extra["equal_to_pillow"] = bool(torch.equal(want, pillow(fs, mode)))
            t = time_host(variants, a.repeats)
            for name, ms in t.items():
                lines.append(line(group, name, b, ms, coded + want.numel(), **extra))
            # the stages alone
            parsed = [I.png_parse(f) for f in fs]
            h, w = parsed[0]["h"], parsed[0]["w"]
            plan = I.png_plan(b, h, w, colour, 8, mode)
            meta, sizes, data, total = I._png_upload([p["stream"] for p in parsed], [plan["size"]] * b, dev)
            raw = torch.empty((b, plan["pitch"]), dtype=torch.uint8, device=dev)
            status = torch.empty((b,), dtype=torch.int32, device=dev)
            out = torch.empty(want.shape, dtype=torch.uint8, device=dev)
            ms1, ms2 = [], []
            for rep in range(a.repeats + 2):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                I.call("w2e_png_inflate", I._p(data), I._p(meta), I._p(sizes), total, b, I._p(raw), plan["pitch"], I._p(status), I.stream_ptr())
                e[1].record()
                I.call("w2e_png_pixels", I._p(raw), plan["pitch"], None, b, h, w, colour, 8, I.PNG_MODES.index(mode), I._p(out), I._p(status), I.stream_ptr())
                e[2].record()
                torch.cuda.synchronize()
                if rep >= 2:
                    ms1.append(e[0].elapsed_time(e[1])), ms2.append(e[1].elapsed_time(e[2]))
            assert int(status.abs().sum()) == 0 and torch.equal(out, want)
            lines.append(line("png_stage" + group[8:], "inflate", b, ms1, sum(len(p["stream"]) for p in parsed) + b * plan["size"]))
            lines.append(line("png_stage" + group[8:], "pixels", b, ms2, b * plan["size"] + want.numel()))
            del raw, out, want


def bench_png_encode(a, lines):
    """to_png against what a caller does today (the pixels to the host, Pillow's PNG encoder on one host core).  Host-clock times of
    whole calls; the two stages on device events, one pair per repeat."""
    import io
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import png_encode_ref as E
    from where2edit_amd import image_io as I
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda", torch.cuda.current_device())

    def pillow(x):
        host = x.cpu().numpy()
        files = []
        for i in range(host.shape[0]):
            buf = io.BytesIO()
            Image.fromarray(host[i, :, :, 0] if host.shape[3] == 1 else host[i]).save(buf, format="PNG")
            files.append(buf.getvalue())
        return files

    labels = torch.from_numpy(np.stack([E.label(512, 512, regions=19, name=f"bench{i}") for i in range(90)]))
    noise = torch.from_numpy(np.stack([E.noise(1024, 1024, name=f"bench{i}") for i in range(8)]))
    cases = [("to_png_rgb_1024", photo_u8(8, 1024, 1024, 0), (1, 8)), ("to_png_label_512", labels, (1, 90)), ("to_png_noise_1024", noise, (8,))]
    for group, images, batches in cases:
        for b in batches:
            x = images[:b].to(dev)
            files = I.to_png(x)
            back = I.from_png(files, mode="raw", stack=True)
            assert torch.equal(back.reshape(x.shape), x)
            variants = {"hip": lambda: I.to_png(x)}
            extra = {"file_bytes": sum(len(f) for f in files)}
            if Image is not None:
                variants["d2h_then_pillow"] = lambda: pillow(x)
                theirs = pillow(x)
                extra["pillow_file_bytes"] = sum(len(f) for f in theirs)
                extra["rows_equal_to_pillow"] = all(zlib_rows(E, f) == zlib_rows(E, g) for f, g in zip(files[:2], theirs[:2]))
            t = time_host(variants, a.repeats)
            for name, ms in t.items():
                lines.append(line(group, name, b, ms, x.numel() + extra["file_bytes"], **extra))
            # the stages alone
            _, h, w, c = x.shape
            plan = I.png_encode_plan(b, h, w, c)
            raw = torch.empty((b, plan["pitch"]), dtype=torch.uint8, device=dev)
            sizes = torch.full((b,), plan["size"], dtype=torch.int64, device=dev)
            out = torch.empty((b, plan["out_pitch"]), dtype=torch.uint8, device=dev)
            lengths = torch.empty((b,), dtype=torch.int64, device=dev)
            work = torch.empty((plan["workspace"],), dtype=torch.uint8, device=dev)
            ms1, ms2 = [], []
            for rep in range(a.repeats + 2):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                I.call("w2e_png_filter", I._p(x), b, h, w, c, I._p(raw), plan["pitch"], I.stream_ptr())
                e[1].record()
                I.call("w2e_png_deflate", I._p(raw), plan["pitch"], I._p(sizes), b, plan["size"], I._p(out), plan["out_pitch"], I._p(lengths), I._p(work),
                       plan["workspace"], I.stream_ptr())
                e[2].record()
                torch.cuda.synchronize()
                if rep >= 2:
                    ms1.append(e[0].elapsed_time(e[1])), ms2.append(e[1].elapsed_time(e[2]))
            coded = int(lengths.sum())
            lines.append(line("png_encode_stage" + group[6:], "filter", b, ms1, x.numel() + b * plan["size"]))
            lines.append(line("png_encode_stage" + group[6:], "deflate", b, ms2, b * plan["size"] + coded, chunks=b * plan["chunks"]))
            del raw, out, work


def zlib_rows(E, f):
    import zlib
    return zlib.decompress(E.idat_payload(f)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--jpeg", action="store_true", help="only the JPEG calls; lines go to --jpeg-out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_io_bench.jsonl"))
    ap.add_argument("--jpeg-out", default=os.path.join(ROOT, "profiles", "jpeg_bench.jsonl"))
    ap.add_argument("--decode", action="store_true", help="only the JPEG decoder; lines go to --decode-out")
    ap.add_argument("--decode-out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.jsonl"))
    ap.add_argument("--png", action="store_true", help="only the PNG decoder; lines go to --png-out")
    ap.add_argument("--png-out", default=os.path.join(ROOT, "profiles", "png_decode_bench.jsonl"))
    ap.add_argument("--png-encode", action="store_true", help="only the PNG encoder; lines go to --png-encode-out")
    ap.add_argument("--png-encode-out", default=os.path.join(ROOT, "profiles", "png_encode_bench.jsonl"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("--repeats must be >= 5: the spread is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("image_io_bench needs the GPU: a host timing says nothing about these kernels")
    lines = []
    with torch.no_grad():
        if a.jpeg:
            bench_jpeg(a, lines)
        elif a.decode:
            bench_decode(a, lines)
        elif a.png:
            bench_png(a, lines)
        elif a.png_encode:
            bench_png_encode(a, lines)
        else:
            bench_calls(a, lines)
            if not a.skip_pipeline:
                bench_pipeline(a, lines)
    for ln in lines:
        print(json.dumps(ln))
    out = a.jpeg_out if a.jpeg else (a.decode_out if a.decode else (a.png_out if a.png else (a.png_encode_out if a.png_encode else a.out)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
