#!/usr/bin/env python3
"""Dev helper (GPU box): what the per-tile denoise does to an adaptively sampled frame (mrt_set_denoise_adaptive) -- the table of
profiles/denoise_tiles_quality.txt.

Cover-glass scene, 640x360 x 1 spp frames.  An adaptive run (State.render_until(adaptive=True), checks every 16 frames) to "no pixel
above 10 %" relative standard error, capped at --max-frames; then, against a 4096-frame uniform render with another seed: the
RMSE of the noisy frame and of its per-tile denoise in the three variance modes, and the mean absolute luminance step between
horizontally / vertically adjacent pixels that lie on two sides of a tile border (and, for scale, between those that do not),
before and after the filter: tiles end at their own frame counts, so the noisy frame's noise level jumps at tile borders.

    python scripts/denoise_tiles_quality.py [--out profiles/denoise_tiles_quality.txt] [--max-frames 8192]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")
import numpy as np          # noqa: E402
import myraytracer_amd as M  # noqa: E402

W, H = 640, 360
MODES = ("accumulated", "prefiltered", "spatial-early")


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def lum(c):
    c = c.astype(np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def border_steps(img):
    """(mean |dL| across tile borders, mean |dL| between neighbours inside a tile)"""
    L = lum(img)
    dx, dy = np.abs(L[:, 1:] - L[:, :-1]), np.abs(L[1:, :] - L[:-1, :])
    bx, by = (np.arange(1, W) % 8) == 0, (np.arange(1, H) % 8) == 0
    across = np.concatenate([dx[:, bx].ravel(), dy[by, :].ravel()])
    inside = np.concatenate([dx[:, ~bx].ravel(), dy[~by, :].ravel()])
    return float(across.mean()), float(inside.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_tiles_quality.txt"))
    ap.add_argument("--max-frames", type=int, default=8192)
    ap.add_argument("--ref-frames", type=int, default=4096)
    a = ap.parse_args()
    spheres, cam = M.scene_cover(1, True)
    with M.State(M.Args(W, H, 1, 50, 1.0), seed=101) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        st.render(a.ref_frames)
        ref = st.read_framebuffer()
    lines = [f"denoise_tiles_quality.py: cover-glass, {W}x{H} x 1 spp, depth 50, seed 7; reference: {a.ref_frames} uniform frames, seed 101"]
    with M.State(M.Args(W, H, 1, 50, 1.0), seed=7) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        frames, rep = st.render_until(0.0, a.max_frames, check_every=16, threshold=0.10, adaptive=True)
        tiles = st.tile_frames()
        lines.append(f"adaptive run to no pixel above rel 0.10 (checks every 16 frames, cap {a.max_frames}): {frames} frames queued, last report at "
                     f"frame {rep['frames_done']}: {rep['above']} pixels above, rel_rmse {rep['rel_rmse']:.5f}")
        lines.append(f"tile frame counts: min {tiles.min()}, median {int(np.median(tiles))}, max {tiles.max()}, {len(np.unique(tiles))} distinct; "
                     f"tile-frames rendered: {int(tiles.sum())} of {int(tiles.size) * int(tiles.max())} of a uniform run to the same maximum")
        noisy = st.read_framebuffer()
        st.set_denoise_adaptive(True)
        across, inside = border_steps(noisy)
        r_across, r_inside = border_steps(ref)
        lines.append("image                      rmse      ratio   mean |dL| across tile borders   inside tiles   across / inside")
        lines.append(f"{'reference':24s} {0.0:8.5f}  {'':>7s}   {r_across:12.5f}                  {r_inside:10.5f}     {r_across / r_inside:6.3f}")
        base = rmse(noisy, ref)
        lines.append(f"{'noisy':24s} {base:8.5f}  {1.0:7.3f}   {across:12.5f}                  {inside:10.5f}     {across / inside:6.3f}")
        for mode in MODES:
            st.set_denoise_variance(mode, 3)
            den = st.read_denoised()
            across, inside = border_steps(den)
            e = rmse(den, ref)
            lines.append(f"{'denoised, ' + mode:24s} {e:8.5f}  {e / base:7.3f}   {across:12.5f}                  {inside:10.5f}     {across / inside:6.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
