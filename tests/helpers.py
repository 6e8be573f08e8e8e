"""Shared helpers for the parity tests: the same call sequence driven through the product
(stitching_amd, HIP) and through the oracle (oracle/oracle.py, CPU restatement)."""
import hashlib

import numpy as np

from stitching_amd import synthetic


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def small_ring(n, w, h, focal_factor=0.75, span=200.0):
    cams = synthetic.ring_cameras(n, w, h, focal_factor=focal_factor, span_deg=span)
    imgs = [synthetic.make_frame(i, w, h) for i in range(n)]
    return imgs, cams


def run_pipeline(mod_warper_cls, mod_blender_cls, imgs, cams, warper_type="spherical", blender_type="multiband",
                 blend_strength=5, masks_fn=None, aspect=1):
    """The linear warp -> blend sequence of the reference (stitching/verbose.py:77-95,176-181;
    tests/stitching_detailed.py:291-419) for either implementation."""
    warper = mod_warper_cls(warper_type)
    warper.set_scale(cams)
    sizes = [(im.shape[1], im.shape[0]) for im in imgs]
    w_imgs = [np.asarray(x) for x in warper.warp_images(imgs, cams, aspect)]
    w_masks = [np.asarray(x) for x in warper.create_and_warp_masks(sizes, cams, aspect)]
    corners, w_sizes = warper.warp_rois(sizes, cams, aspect)
    feed_masks = masks_fn(w_masks, corners, w_sizes) if masks_fn else w_masks
    blender = mod_blender_cls(blender_type, blend_strength)
    blender.prepare(corners, w_sizes)
    for img, mask, corner in zip(w_imgs, feed_masks, corners):
        blender.feed(img, mask, corner)
    pano, pmask = blender.blend()
    return dict(w_imgs=w_imgs, w_masks=w_masks, corners=corners, sizes=w_sizes, pano=np.asarray(pano),
                pmask=np.asarray(pmask), blender=blender)


class StripRecorder:
    """Transport stand-in, pass 1 of a sharded job executed rank after rank in ONE process: keeps what the rank sends (host
    copies) and hands back zero-filled buffers of the planned sizes (the bands of this pass are discarded)."""

    def __init__(self, ctx):
        self.ctx, self.sent, self.recvs = ctx, [], []

    def start(self, sends, recvs, ctx=None):
        self.sent = [(dst, np.asarray(p).reshape(-1)[:nb].copy()) for dst, p, nb in sends]
        self.recvs = recvs

    def finish(self, ctx=None):
        from stitching_amd.distributed import flat_device_buffer

        return [flat_device_buffer(self.ctx, np.zeros(nb, np.uint8)) for _, nb in self.recvs]


class StripReplay:
    """Pass 2: the strips the other ranks recorded arrive as this rank's incoming ones, in plan order."""

    def __init__(self, ctx, inbox):
        self.ctx, self.inbox, self.recvs = ctx, inbox, []

    def start(self, sends, recvs, ctx=None):
        self.recvs = recvs

    def finish(self, ctx=None):
        from stitching_amd.distributed import flat_device_buffer

        out = []
        for src, nb in self.recvs:
            a = self.inbox[src].pop(0)
            assert a.size == nb
            out.append(flat_device_buffer(self.ctx, a))
        return out


def run_sharded_job_in_one_process(ctx, frames, cams, world, per_rank, **job_kw):
    """Every rank of a ShardedStitchJob (as bench.py builds it for N > 1) executed one after the other on one GPU: pass 1
    records each rank's outgoing strips, pass 2 replays them as the incoming ones.  -> (panorama, mask, jobs): the
    concatenated bands of pass 2."""
    from stitching_amd.distributed import ShardedStitchJob

    jobs, recs = [], []
    for r in range(world):
        rec = StripRecorder(ctx)
        job = ShardedStitchJob(frames[r * per_rank:(r + 1) * per_rank], cams[r * per_rank:(r + 1) * per_rank], cams, r, world,
                               ctx=ctx, transport=rec, **job_kw)
        job.plan()
        out = job.run()
        del out
        jobs.append(job)
        recs.append(rec)
    bands = []
    for r in range(world):
        inbox = {src: [a for dst, a in recs[src].sent if dst == r] for src in range(world) if src != r}
        jobs[r].transport = StripReplay(ctx, inbox)
        bands.append(tuple(np.asarray(a) for a in jobs[r].run()))
    pano = np.concatenate([b[0] for b in bands], axis=1)
    mask = np.concatenate([b[1] for b in bands], axis=1)
    return pano, mask, jobs


def weight_pyramid_of_export(packed, rect, nb):
    """the fp32 weight planes W_0 .. W_nb out of a packed contribution strip (csrc/stx_blend_host.cpp mb_contrib_layout: per level three
    int16 planes, row pitch a multiple of 32 samples, then the weights, pitch a multiple of 16; every section on a 256-byte boundary)"""
    raw = np.asarray(packed).reshape(-1)
    w, h = rect[2], rect[3]
    up = lambda v, a: (v + a - 1) // a * a  # noqa: E731
    off, out = 0, []
    for i in range(nb + 1):
        lw, lh = max(w >> i, 1), max(h >> i, 1)
        off = up(off + up(lw, 32) * lh * 3 * 2, 256)
        ws = up(lw, 16)
        out.append(raw[off:off + ws * lh * 4].view(np.float32).reshape(lh, ws)[:, :lw].copy())
        off = up(off + ws * lh * 4, 256)
    return out


def many_images_feeds(n):
    """-> (images, masks, corners): n images of 1100 x 96 stacked over the same panorama pixels with binary masks — checkerboards, flat
    and random images, ragged left edges, every fifth mask salt and pepper (test_gpu_parity.test_blend_many_images_over_the_same_pixels;
    classified in tests/test_constructed_multiband.py)"""
    rng = np.random.default_rng(1000 + n)
    w, h = 1100, 96
    yy, xx = np.mgrid[0:h, 0:w]
    imgs, masks, corners = [], [], []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            im = np.where(((xx + yy + k) & 1)[..., None] == 1, 255, 0).astype(np.uint8).repeat(3, axis=2)
        elif kind == 1:
            im = np.full((h, w, 3), 255 if k % 8 == 1 else 0, np.uint8)
        else:
            im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = np.full((h, w), 255, np.uint8)
        x0, x1 = int(rng.integers(0, 200)), int(rng.integers(w - 200, w + 1))
        m[:, :x0] = 0
        m[:, x1:] = 0
        ragged = rng.integers(0, 12, h)
        for y in range(h):  # ragged left edge: the count changes from pixel to pixel within a lane's patch
            m[y, x0:x0 + int(ragged[y])] = 0
        if k % 5 == 4:
            m[rng.integers(0, 2, (h, w)) == 0] = 0  # a salt-and-pepper mask
        imgs.append(im)
        masks.append(m)
        corners.append((int(rng.integers(0, 9)) if k else 0, int(rng.integers(0, 5)) if k else 0))
    return imgs, masks, corners


def sparse_masks(kind, masks, rng):
    """warped masks thinned to islands at the 512-column tile seams, single dots (image 1: nothing), grey islands, or one-pixel lines
    along the rectangle's edges (test_gpu_parity.test_blend_sparse_masks_bit_exact; classified in tests/test_constructed_multiband.py)"""
    out = []
    for k, m in enumerate(masks):
        hh, ww = m.shape
        z = np.zeros_like(m)
        if kind == "islands":
            for x in (0, 500, 1016, ww - 40):
                y = int(rng.integers(0, hh - 30))
                z[y:y + 24, x:x + 33] = m[y:y + 24, x:x + 33]
        elif kind == "empty_and_dots":
            if k != 1:  # image 1: nothing at all
                for (y, x) in ((0, 0), (hh - 1, ww - 1), (hh // 2, 511), (hh // 2 + 1, 512), (3, ww // 3)):
                    z[y, x] = 255
        elif kind == "grey_islands":
            for _ in range(5):
                y, x = int(rng.integers(0, hh - 20)), int(rng.integers(0, ww - 80))
                z[y:y + 17, x:x + 70] = rng.integers(0, 256, (17, 70), dtype=np.uint8)
        else:
            z[0, :] = 255; z[hh - 1, :] = 255; z[:, 0] = 255; z[:, ww - 1] = 255
            z &= m if k % 2 else z
        out.append(z)
    return out
