#!/usr/bin/env python3
"""The uint8 movers (curla_random_shift_u8, curla_cutout_u8, curla_translate_u8, curla_dihedral_u8, curla_grayscale_u8,
curla_affine_u8; csrc/u8_mover.h, csrc/affine.h, augment.hip) against
one another and against a plain device-to-device copy, and whole updates with their augmentations:
python tools/u8_mover_bench.py [--kernels shift,cutout,translate,flip,rotate,grey,affine,copy] [--kinds] [--fused] [--launches K]
                               [--augs identity,random_shift,cutout_color,translate,flip,rotate,grayscale,affine] [--no-updates]
Kernels: one launch for a 3B minibatch (obs | next_obs | pos from a double ring, period 2B, as ReplayBuffer issues it),
B = 512, so n = 1536, at 84 x 84 x 9 and 90 x 160 x 9: the shift (pad 4), the cutout (boxes drawn by RandomCutout's defaults,
min_cut 10, max_cut 30, random colours), the translate onto a canvas 8 pixels larger per side length (-> 92 x 92 and
98 x 168, offsets in [0, 8]^2) and ``copy_`` of a uint8 tensor of the frame's 3B * frame bytes.  ``flip``: every sample
mirrored (its worst case; ``flip-mix``, the drawn mix at p = 0.5, comes with it); ``rotate``: every sample transposing
(codes 5 and 6, the worst case; on a frame that is not square every sample turned by 180 degrees), with ``rotate-mix``,
the mix RandomRotate draws at p = 0.3; ``grey``: every sample greyed, with ``grey-mix`` at p = 0.3; ``affine``: the words
RandomAffine draws with its defaults (10 degrees, scale 0.9 .. 1.1, 5 % shift, edge fill), with ``affine-id`` (the identity
words: the same loads and blends, the smallest source box) and ``affine-45`` (every sample turned by 45 degrees: the
largest box).  ``--kinds`` adds the
translate onto a canvas of the frame's own size (a plain gather: every group is an inside group, one load and one store),
to tell what the margin and mixed groups cost.  ``--fused`` adds, for each of the three movers of curla_move_cutout_u8
(the crop to 76 x 76 and 80 x 144 -- output frames of whole 16-byte groups --, the shift, the translate), three forms: the
plain mover (``crop``; the shift and the translate are the kernels above), the fused launch with boxes drawn for the
OUTPUT frame (``crop+cutout`` ...) and the two launches it replaces, the mover into a scratch and curla_cutout_u8 over that
scratch (``crop,cutout`` ...); the ratios fused / plain and fused / two launches are printed.  The selected forms alternate; each sample is 10 back-to-back repetitions
between two HIP events (launch gaps hidden behind the queue); medians of 15 samples (``--launches K``: K / 10) are printed
with min - max and the rates of bytes WRITTEN and of bytes read + written, then the ratios of the times to the copy's and
to the shift's, the latter also as bytes written per second.
For kernel times proper run it under the profiler, kernel trace only, in a run of its own, and read
u8_mover_kernel<ShiftOp>, u8_mover_kernel<TrOp> and cutout_u8_kernel from kernel_stats.csv (tools/summarize_rocprof.py); leave ``--kinds`` out
there, the statistics go by kernel name:
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/u8_mover_bench.py --no-updates
Updates (tools/host_overhead.py's loop): 60 updates back to back, three times, eager and replayed from update graphs,
with each of ``--augs`` at the same geometries (names that begin with ``random_crop`` crop to 76 x 76 and 80 x 144)."""
import argparse, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import curla_amd
from curla_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--kernels", default="shift,cutout,translate,copy")
ap.add_argument("--kinds", action="store_true")
ap.add_argument("--fused", action="store_true")
ap.add_argument("--launches", type=int, default=150)
ap.add_argument("--augs", default="identity,random_shift,cutout_color,translate")
ap.add_argument("--no-updates", action="store_true")
args = ap.parse_args()
REP = 10
SAMPLES = max(1, args.launches // REP)
GEOMETRIES = ((84, 84, 9, 512), (90, 160, 9, 512))
CROPS = {(84, 84): (76, 76), (90, 160): (80, 144)}
PAD, CAP = 4, 4096
dev = torch.device("cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3  # us


for (H, W, C, B) in GEOMETRIES:
    Ho, Wo, n = H + 2 * PAD, W + 2 * PAD, 3 * B
    frame, oframe = H * W * C, Ho * Wo * C
    store = torch.zeros(2 * CAP * frame + 32, dtype=torch.uint8, device=dev)
    store.random_(0, 256)
    ring = store[:2 * CAP * frame].view(2 * CAP, H, W, C)
    idx = torch.randint(0, CAP, (B,), device=dev)
    idx2 = torch.cat([idx, idx + CAP])
    dy = torch.randint(0, 2 * PAD + 1, (n,), device=dev, dtype=torch.int32)
    dx = torch.randint(0, 2 * PAD + 1, (n,), device=dev, dtype=torch.int32)
    ty = torch.randint(0, Ho - H + 1, (n,), device=dev, dtype=torch.int32)
    tx = torch.randint(0, Wo - W + 1, (n,), device=dev, dtype=torch.int32)
    np.random.seed(1)
    y0, x0, bh, bw, rgb = curla_amd.RandomCutout((H, W), color=True).draw_boxes(n)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    box = [i32(y0), i32(x0), i32(bh | (bw << 16)), i32(rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16))]
    out = torch.zeros(n * oframe + 32, dtype=torch.uint8, device=dev)
    out_v, out_tv = out[:n * frame].view(n, H, W, C), out[:n * oframe].view(n, Ho, Wo, C)
    src = torch.zeros(n * frame, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    forms = {  # name: (launch, bytes written, what it is)
        "shift": (lambda: ops.random_shift_u8(ring, idx2, 2 * B, dy, dx, PAD, n, out_v), n * frame, f"pad {PAD}"),
        "cutout": (lambda: ops.cutout_u8(ring, idx2, 2 * B, *box, n, out_v), n * frame,
                   f"{100 * float((bh * bw).sum()) / (n * H * W):.1f} % of the bytes inside a box"),
        "translate": (lambda: ops.translate_u8(ring, idx2, 2 * B, ty, tx, n, out_tv), n * oframe, f"-> {Ho}x{Wo}"),
        "gather": (lambda: ops.translate_u8(ring, idx2, 2 * B, ty, tx, n, out_v), n * frame,
                   f"translate -> {H}x{W}, inside groups only"),
        "copy": (lambda: dst.copy_(src), n * frame, "copy_"),
    }
    np.random.seed(3)
    turned = np.where(np.arange(n) % 2, 5, 6) if H == W else np.full(n, 3)
    words = {"flip": (np.ones(n), "every sample mirrored"),
             "flip-mix": (curla_amd.RandomFlip((H, W)).draw_index_words(n)[0], "the draw at p = 0.5"),
             "rotate": (turned, "every sample transposing" if H == W else "every sample turned by 180 degrees"),
             "rotate-mix": (curla_amd.RandomRotate((H, W)).draw_index_words(n)[0], "the draw at p = 0.3"),
             "grey": (np.ones(n), "every sample greyed"),
             "grey-mix": (curla_amd.RandomGrayscale((H, W)).draw_index_words(n)[0], "the draw at p = 0.3")}
    for k, (w, what) in words.items():
        op = ops.grayscale_u8 if k.startswith("grey") else ops.dihedral_u8
        forms[k] = (lambda op=op, w=i32(w): op(ring, idx2, 2 * B, w, n, out_v), n * frame,
                    f"{what}: {100 * float((np.asarray(w) != 0).mean()):.0f} % of the samples transformed")
    aff = curla_amd.RandomAffine((H, W))
    aff_words = {"affine": (aff.draw_index_words(n), "the draw at the defaults"),
                 "affine-id": (np.array(aff.IDENTITY_WORDS)[:, None].repeat(n, 1), "the identity words"),
                 "affine-45": (aff.words(np.full(n, np.pi / 4), 1.0, 0.0, 0.0), "every sample turned by 45 degrees")}
    for k, (w, what) in aff_words.items():
        forms[k] = (lambda w=[i32(x) for x in w]: ops.affine_u8(ring, idx2, 2 * B, w, 1, n, out_v), n * frame, what)
    names = []
    for k in args.kernels.split(","):
        names += ([k, k + "-mix"] if k in ("flip", "rotate", "grey") else [k, k + "-id", k + "-45"] if k == "affine"
                  else [k] if k else [])
    names += ["gather"] if args.kinds else []
    if args.fused:
        Hc, Wc = CROPS[(H, W)]
        h1 = torch.randint(0, H - Hc + 1, (n,), device=dev, dtype=torch.int32)
        w1 = torch.randint(0, W - Wc + 1, (n,), device=dev, dtype=torch.int32)
        mid = torch.zeros(n * oframe + 32, dtype=torch.uint8, device=dev)  # the scratch between the two launches
        movers = {"crop": (ops.MOVE_CROP, h1, w1, 0, (Hc, Wc)), "shift": (ops.MOVE_SHIFT, dy, dx, PAD, (H, W)),
                  "translate": (ops.MOVE_TRANSLATE, ty, tx, 0, (Ho, Wo))}
        for k, (code, a, b, pad, (h, w)) in movers.items():
            np.random.seed(2)
            y0, x0, bh, bw, rgb = curla_amd.RandomCutout((h, w), color=True).draw_boxes(n)
            bx = [i32(y0), i32(x0), i32(bh | (bw << 16)), i32(rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16))]
            o_v, m_v = out[:n * h * w * C].view(n, h, w, C), mid[:n * h * w * C].view(n, h, w, C)
            what = f"-> {h}x{w}, {100 * float((bh * bw).sum()) / (n * h * w):.1f} % of the bytes inside a box"

            def plain(code=code, a=a, b=b, pad=pad, to=o_v):
                ops.move_cutout_u8(ring, idx2, 2 * B, code, a, b, pad, None, n, to)

            def fused(code=code, a=a, b=b, pad=pad, bx=bx, to=o_v):
                ops.move_cutout_u8(ring, idx2, 2 * B, code, a, b, pad, bx, n, to)

            def two(code=code, a=a, b=b, pad=pad, bx=bx, m_v=m_v, to=o_v):
                ops.move_cutout_u8(ring, idx2, 2 * B, code, a, b, pad, None, n, m_v)
                ops.cutout_u8(m_v, None, n, *bx, n, to)
            forms.setdefault(k, (plain, n * h * w * C, f"-> {h}x{w}"))
            forms[k + "+cutout"] = (fused, n * h * w * C, what + ", one launch")
            forms[k + ",cutout"] = (two, n * h * w * C, what + ", two launches")
            names += [x for x in (k, k + "+cutout", k + ",cutout") if x not in names]
    for _ in range(3):
        for k in names:
            forms[k][0]()
    torch.cuda.synchronize()
    t = {k: [] for k in names}
    for _ in range(SAMPLES):
        for k in names:
            t[k].append(timed(forms[k][0]))
    med = {k: statistics.median(t[k]) for k in names}
    rate = {k: forms[k][1] / med[k] / 1e6 for k in names}  # TB/s written
    for k in names:
        print(f"{H}x{W}x{C} n={n} {k:9s} ({forms[k][2]}; {forms[k][1] / 1e6:.1f} MB written, {n * frame / 1e6:.1f} MB source): "
              f"median {med[k]:.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}), {rate[k]:.2f} TB/s written, "
              f"{(forms[k][1] + n * frame) / med[k] / 1e6:.2f} TB/s read + written", flush=True)
    ratios = [f"{k} / copy {med[k] / med['copy']:.3f}" for k in names if k != "copy" and "copy" in med]
    ratios += [f"{k} / shift {med[k] / med['shift']:.3f} (bytes written per second: {rate[k] / rate['shift']:.3f})"
               for k in names if k not in ("copy", "shift") and "shift" in med]
    if args.fused:
        ratios += [f"{k}+cutout / {k} {med[k + '+cutout'] / med[k]:.3f}, {k}+cutout / {k},cutout "
                   f"{med[k + '+cutout'] / med[k + ',cutout']:.3f}" for k in movers]
    if ratios:
        print(f"{H}x{W}x{C} n={n} ratios of the medians: " + ", ".join(ratios), flush=True)
    del store, ring, out, out_v, out_tv, src, dst, forms
    if args.fused:
        del mid, movers, plain, fused, two, o_v, m_v

if args.no_updates:
    sys.exit(0)


class L:
    def log(self, *a, **k):
        pass


for (H, W, C, B) in GEOMETRIES:
    for graphs in (False, True):
        for name in [a for a in args.augs.split(",") if a]:
            curla_amd.set_seed_everywhere(1)
            aug = curla_amd.make_augmentor(name, (H, W), CROPS[(H, W)] if name.startswith("random_crop") else None)
            out_hw = getattr(aug, "output_shape", None) or (H, W)
            agent = curla_amd.CurlSacAgent((C,) + tuple(out_hw), (2,), dev, aug, hidden_dim=1024, log_interval=10 ** 9)
            rb = curla_amd.ReplayBuffer((C, H, W), (2,), 20000, B, dev, aug)
            rb._obs_store.random_(0, 256); rb._next_store.random_(0, 256)
            rb.actions.uniform_(-1, 1); rb.rewards.normal_(); rb.not_dones.fill_(1.0); rb.idx, rb.full = 0, True
            if graphs:
                agent.enable_update_graphs(rb)
            step = 1  # (never a logging step)
            for _ in range(20):
                agent.update(rb, L(), step); step += 1
            times = []
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(60):
                    agent.update(rb, L(), step); step += 1
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / 60 * 1e3)
            print(f"{H}x{W}x{C} B={B} {name:12s} graphs {graphs}: 60 updates back to back, median {statistics.median(times):.3f} "
                  f"ms/update (min {min(times):.3f}, max {max(times):.3f})", flush=True)
            del agent, rb
            torch.cuda.empty_cache()
