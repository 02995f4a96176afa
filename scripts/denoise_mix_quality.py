#!/usr/bin/env python3
"""Dev helper (host only): what the denoiser's blend with the accumulation (mrt_set_denoise_mix) buys, and the default gain -- the
table of profiles/denoise_mix_quality.txt.  RMSE of the noisy accumulation, of its denoised preview and of the blend at several
gains -- the same frames -- against a long render with another seed, on the cover scene without glass, 1 spp frames, depth 50,
uniform accumulation, default denoise parameters, in the three variance modes (spatial_frames 3).

Everything runs on the host through the float32 references the kernels are held to bit for bit: the oracle's frames
(tests/test_gpu_parity.py), tests/noise_ref.py's accumulation, tests/denoise_ref.py's guides, and tests/denoise_mix_ref.py's filter
and blend (tests/test_gpu_denoise_mix.py).
   python scripts/denoise_mix_quality.py [--out FILE] [--ref-frames N] [w h]
The default gain is the one with the smallest worst case of rmse_blend / min(rmse_noisy, rmse_denoised) over the whole table; the
smaller gain wins a tie."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import myraytracer_amd as M
from oracle import pyoracle as O
import denoise_mix_ref as R
from denoise_var_ref import MODES, variance_of

GAINS = (1.0, 1.5, 2.0, 3.0)
SEEDS = (7, 8)
COUNTS = (2, 3, 4, 8, 16, 32, 64, 128, 256, 512)
REF_SEED = 101


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    ref_frames = int(argv[argv.index("--ref-frames") + 1]) if "--ref-frames" in argv else 1024
    pos = [x for i, x in enumerate(argv) if not x.startswith("--") and (i == 0 or argv[i - 1] not in ("--out", "--ref-frames"))]
    w, h = (int(pos[0]), int(pos[1])) if pos else (320, 192)
    sp, cam = M.scene_cover(1, False)
    guides = R.host_guides(O, sp, M.camera_derive(cam), w, h)
    ref = R.oracle_accumulations(O, sp, cam, w, h, REF_SEED, [ref_frames], noise=False)[ref_frames][0]
    lines, worst = [], {g: (0.0, None) for g in GAINS}
    for seed in SEEDS:
        acc = R.oracle_accumulations(O, sp, cam, w, h, seed, COUNTS)
        for mi, mode in enumerate(MODES):
            lines.append(f"cover {w}x{h} x 1 spp, seed {seed}, {mode}, spatial_frames 3, default parameters, reference {ref_frames} frames of seed {REF_SEED}")
            lines.append("frames  rmse_noisy  rmse_denoised  " + "  ".join(f"gain {g:<4g}" for g in GAINS) +
                         "   blend / min(noisy, denoised): " + "  ".join(f"{g:<5g}" for g in GAINS))
            for n in COUNTS:
                fb, S, K = acc[n]
                fu = R.filtered(fb, S, K, guides, None, variance_of(mi, n))
                noisy, den = R.rmse(fb, ref), R.rmse(fu, ref)
                mix = [R.rmse(R.blend(fb, S, fu, K, guides["index"], g), ref) for g in GAINS]
                best = min(noisy, den)
                for g, x in zip(GAINS, mix):
                    if x / best > worst[g][0]:
                        worst[g] = (x / best, (seed, mode, n))
                lines.append(f"{n:6d}  {noisy:10.5f}  {den:13.5f}  " + "  ".join(f"{x:9.5f}" for x in mix) +
                             "                                   " + "  ".join(f"{x / best:5.3f}" for x in mix))
                print(lines[-1], flush=True)
    lines.append("")
    lines.append("worst case of blend / min(noisy, denoised) over the table, per gain:")
    for g in GAINS:
        r, (seed, mode, n) = worst[g]
        lines.append(f"  gain {g:<4g} {r:6.4f}   (seed {seed}, {mode}, {n} frames)")
    chosen = min(GAINS, key=lambda g: (round(worst[g][0], 4), g))
    lines.append(f"chosen default gain: {chosen:g}" + ("" if worst[chosen][0] < 1.05 else "   (NO gain keeps the worst case under 1.05)"))
    text = "\n".join(lines) + "\n"
    print(text[text.index("worst case"):])
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
