"""JPEG decode: Pillow on one host thread against the GPU path (data/jpeg.py + csrc/jpeg.hip), on the same seeded files.

    python tools/jpeg_decode_bench.py --out profiles/jpeg_decode_bench.json

Files: --images (512) photo-like 800 x 800 frames (a smooth field plus noise) at q75 4:2:0, q90 4:2:0 and q95 4:4:4, written to a
temporary directory, plus one 4000 x 3000 q90 4:2:0 file.  Arms, alternating in both orders inside one process, --reps (7)
repetitions each after one warm-up, medians reported:
  (a) Pillow: open + convert("RGB") + load of --pillow-images (64) of the files on one thread -> images/s
  (b) the GPU path: host microseconds per image on one thread for read + parse_jpeg (which unstuffs and cuts the scan) and for the
      batch tables (layout + pack); device-event times of the host-to-device copy, of ia_jpeg_entropy and of ia_jpeg_reconstruct
      summed over the chunks of the batch; bytes copied per image; pass-B rounds (median, maximum)
The images/s of (b) takes its host part and its GPU stages in series.  Every decoded frame of the first repetition is compared with
Pillow's.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def photo(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 3), dtype=np.float32)
    for c in range(3):
        f = rng.uniform(0.01, 0.08, size=4).astype(np.float32)
        ph = rng.uniform(0, 6.28, size=2).astype(np.float32)
        img[:, :, c] = 128 + 70 * np.sin(xx * f[0] + yy * f[1] + ph[0]) + 40 * np.cos(xx * f[2] - yy * f[3] + ph[1])
    img += rng.standard_normal(size=img.shape, dtype=np.float32) * 12
    return np.clip(img, 0, 255).astype(np.uint8)


def write_files(directory, n, w, h, configs):
    from PIL import Image
    paths = {name: [] for name, _, _ in configs}
    for i in range(n):
        im = Image.fromarray(photo(w, h, 1000 + i))
        for name, q, samp in configs:
            p = os.path.join(directory, f"{name}_{w}x{h}_{i}.jpg")
            im.save(p, "JPEG", quality=q, subsampling=samp)
            paths[name].append(p)
    return paths


def pillow_arm(paths):
    from PIL import Image
    t = time.perf_counter()
    for p in paths:
        im = Image.open(p).convert("RGB")
        im.load()
    return len(paths) / (time.perf_counter() - t)


def gpu_arm(dec, paths, bits, check=False):
    import torch
    from item_alignment_amd.data.jpeg import parse_jpeg
    t0 = time.perf_counter()
    plans = []
    for p in paths:
        plan = parse_jpeg(np.fromfile(p, dtype=np.uint8))
        assert plan is not None, p
        plans.append(plan)
    host_us = (time.perf_counter() - t0) * 1e6 / len(paths)
    batch_s, h2d_ms, ent_ms, rec_ms, h2d_bytes, rounds, status, frames = 0.0, 0.0, 0.0, 0.0, 0, [], [], []
    for idxs in dec.chunks(plans):
        sub = [plans[i] for i in idxs]
        t1 = time.perf_counter()
        lay = dec.layout(sub, bits)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        dev, ptrs, nbytes = dec._upload(lay)
        batch_s += time.perf_counter() - t1
        ev[1].record()
        coef, stat = dec.launch_entropy(lay, ptrs, len(sub), bits)
        ev[2].record()
        out = dec.reconstruct(sub, coef, lay, ptrs)
        ev[3].record()
        torch.cuda.synchronize()
        h2d_ms += ev[0].elapsed_time(ev[1])
        ent_ms += ev[1].elapsed_time(ev[2])
        rec_ms += ev[2].elapsed_time(ev[3])
        h2d_bytes += nbytes
        st = stat.cpu().numpy()
        status += st[0].tolist()
        rounds += st[1].tolist()
        if check:
            frames += [f.cpu().numpy() for f in out]
        del out, dev
    assert not any(status), "an image came back with a non-zero status"
    if check:
        from PIL import Image
        for p, f in zip(paths, frames):
            assert np.array_equal(f, np.array(Image.open(p).convert("RGB"))), p
    return dict(host_parse_us_per_image=host_us, host_batch_us_per_image=batch_s * 1e6 / len(paths), h2d_ms=h2d_ms, entropy_ms=ent_ms,
                reconstruct_ms=rec_ms, h2d_bytes_per_image=h2d_bytes / len(paths), rounds_median=float(statistics.median(rounds)),
                rounds_max=int(max(rounds)), chunks=len(dec.chunks(plans)))


def measure(dec, paths, bits, reps, n_pillow):
    n = len(paths)
    gpu_arm(dec, paths, bits, check=True)                                  # warm-up of both arms; every frame compared with Pillow's
    pillow_arm(paths[:n_pillow])
    a, b = [], []
    for r in range(reps):
        for arm in ("ab", "ba")[r % 2]:
            if arm == "a":
                a.append(pillow_arm(paths[:n_pillow]))
            else:
                b.append(gpu_arm(dec, paths, bits))
    med = {k: statistics.median(x[k] for x in b) for k in b[0]}
    per_image_us = med["host_parse_us_per_image"] + med["host_batch_us_per_image"] + (med["h2d_ms"] + med["entropy_ms"] + med["reconstruct_ms"]) * 1e3 / n
    pil = statistics.median(a)
    return dict(images=n, file_kb=sum(os.path.getsize(p) for p in paths) / n / 1024, pillow_images_per_s=pil, pillow_images_per_s_min_max=[min(a), max(a)],
                gpu=med, gpu_entropy_ms_min_max=[min(x["entropy_ms"] for x in b), max(x["entropy_ms"] for x in b)],
                gpu_path_images_per_s_in_series=1e6 / per_image_us, ratio_to_pillow_one_thread=1e6 / per_image_us / pil, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--pillow-images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--subseq_bits", type=int, default=1024)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs the GPU")
    import PIL
    from item_alignment_amd.data.jpeg import GpuJpegDecoder
    dec = GpuJpegDecoder(torch.device("cuda:0"))
    configs = [("q75_420", 75, "4:2:0"), ("q90_420", 90, "4:2:0"), ("q95_444", 95, "4:4:4")]
    result = dict(device=torch.cuda.get_device_name(0), pillow=PIL.__version__, subseq_bits=args.subseq_bits, frame=f"{args.size}x{args.size}", rows={})
    with tempfile.TemporaryDirectory() as d:
        paths = write_files(d, args.images, args.size, args.size, configs)
        for name, _, _ in configs:
            result["rows"][name] = measure(dec, paths[name], args.subseq_bits, args.reps, min(args.pillow_images, args.images))
            print(name, json.dumps(result["rows"][name]), flush=True)
        if not args.no_large:
            big = write_files(d, 1, 4000, 3000, [("q90_420", 90, "4:2:0")])["q90_420"]
            result["rows"]["one_4000x3000_q90_420"] = measure(dec, big, args.subseq_bits, args.reps, 1)
            print("one_4000x3000_q90_420", json.dumps(result["rows"]["one_4000x3000_q90_420"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (round(v["pillow_images_per_s"], 1), round(v["gpu_path_images_per_s_in_series"], 1)) for k, v in result["rows"].items()}))


if __name__ == "__main__":
    main()
