"""Seeded synthetic weights and inputs (numpy PCG64, platform independent).

No trained COTR checkpoint nor ImageNet ResNet-50 weights exist offline
(SURVEY.md fact 0.5), so the benchmark and the parity tests run on random
weights.  The distributions follow the reference's initialisers (kaiming
fan-out for convs as torchvision does, xavier-uniform for every transformer
matrix as ``COTR/models/transformer.py:42-45`` does, torch's Linear default for
``corr_embed``) but ALSO randomise every bias, every LayerNorm affine and all
four FrozenBN buffers, so that a kernel which drops or misplaces any of them
fails parity.  The last BN of each bottleneck gets a smaller gain so the
residual stream stays O(1) like in a trained network.
"""
import math
from collections import OrderedDict

import numpy as np

from ..models.spec import state_spec


def synth_state_dict(seed=0, attn_gain=1.0, as_torch=True, **spec_kw):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = OrderedDict()
    for name, (shape, kind) in state_spec(**spec_kw).items():
        if kind == 'conv':
            fan_out = shape[0] * shape[2] * shape[3]
            w = rng.standard_normal(shape) * math.sqrt(2.0 / fan_out)
        elif kind in ('mat', 'mlp_w'):
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            bound = math.sqrt(6.0 / (fan_in + fan_out)) if kind == 'mat' else 1.0 / math.sqrt(fan_in)
            w = rng.uniform(-bound, bound, shape)
            if name.endswith('in_proj_weight') and attn_gain != 1.0:
                w[: 2 * shape[1]] *= attn_gain  # sharpen q and k -> peakier softmax
        elif kind == 'bias':
            w = 0.05 * rng.standard_normal(shape)
        elif kind == 'mlp_b':
            w = rng.uniform(-1.0 / 16.0, 1.0 / 16.0, shape)
        elif kind == 'ln_w':
            w = rng.uniform(0.8, 1.2, shape)
        elif kind == 'ln_b':
            w = 0.05 * rng.standard_normal(shape)
        elif kind == 'bn_w':
            w = rng.uniform(0.8, 1.2, shape)
        elif kind == 'bn_w_last':
            w = rng.uniform(0.15, 0.35, shape)
        elif kind == 'bn_b':
            w = 0.1 * rng.standard_normal(shape)
        elif kind == 'bn_rm':
            w = 0.1 * rng.standard_normal(shape)
        elif kind == 'bn_rv':
            w = rng.uniform(0.75, 1.25, shape)
        else:
            raise AssertionError(kind)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    if as_torch:
        import torch
        return OrderedDict((k, torch.from_numpy(v)) for k, v in out.items())
    return out


def synth_inputs(batch, queries, seed=1, as_torch=True):
    """img ~ N(0,1) [B,3,256,512] (ImageNet-normalised pixels have that range),
    queries ~ U[0,1)^2 [B,Q,2] (x<0.5: left image, x>=0.5: right image)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.standard_normal((batch, 3, 256, 512)).astype(np.float32)
    q = rng.random((batch, queries, 2)).astype(np.float32)
    if as_torch:
        import torch
        return torch.from_numpy(img), torch.from_numpy(q)
    return img, q


def _ray_plane_depth(H, W, K, c2w, normal, offset):
    """(depth along the camera's z of the plane normal . X = offset seen through every pixel centre (x, y), world hit points):
    analytic ray-plane intersection in float64; pixel (x, y) looks along Kinv (x, y, 1), whose z is 1, so the ray parameter
    IS the depth"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    origin = c2w[:3, 3]
    t = (offset - normal @ origin) / (rays @ normal)
    return t, origin + rays * t[..., None]


def synth_captures(seed, H, W):
    """A seeded two-view RGB-D scene -> (query, nn), each a ``cotr_amd.data.Capture`` of numpy arrays (image uint8 [H, W, 3],
    depth float32 [H, W], K, c2w float64): a tilted background plane, a nearer plane patch that occludes part of it, holes
    in the depth (rectangles and single pixels, 0 as in MegaDepth), two poses a few degrees and a fraction of the depth
    apart, and an image textured by the world position of what each pixel sees.  Depth is exact ray-plane intersection in
    float64, cast to float32."""
    from ..data import Capture
    rng = np.random.Generator(np.random.PCG64(seed))
    f = 0.9 * max(H, W)
    K = np.array([[f, 0.0, W / 2.0], [0.0, f * 1.02, H / 2.0], [0.0, 0.0, 1.0]])
    planes = [(np.array([0.18, -0.12, 1.0]), 8.0 + rng.uniform(-0.5, 0.5), None),
              (np.array([-0.25, 0.1, 1.0]), 5.0 + rng.uniform(-0.3, 0.3), (rng.uniform(-0.6, 0.2), rng.uniform(-0.4, 0.2), 1.4, 1.1))]

    def pose(angles, t):
        ax, ay, az = np.deg2rad(angles)
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        m = np.eye(4)
        m[:3, :3] = rz @ ry @ rx
        m[:3, 3] = t
        return m

    poses = [pose(rng.uniform(-1, 1, 3), rng.uniform(-0.05, 0.05, 3)),
             pose(np.array([2.0, -5.0, 1.5]) + rng.uniform(-1, 1, 3), np.array([0.9, 0.15, 0.4]) + rng.uniform(-0.1, 0.1, 3))]
    caps = []
    for c2w in poses:
        depth = np.full((H, W), np.inf)
        hit = np.zeros((H, W, 3))
        for normal, offset, rect in planes:
            normal = normal / np.linalg.norm(normal)
            t, pts = _ray_plane_depth(H, W, K, c2w, normal, offset)
            ok = (t > 0) & (t < depth)
            if rect is not None:
                ok &= (np.abs(pts[..., 0] - rect[0]) < rect[2]) & (np.abs(pts[..., 1] - rect[1]) < rect[3])
            depth = np.where(ok, t, depth)
            hit = np.where(ok[..., None], pts, hit)
        depth = np.where(np.isfinite(depth), depth, 0.0)
        for _ in range(3):                                             # holes: rectangles ...
            h0, w0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            depth[h0:h0 + max(1, H // 9), w0:w0 + max(1, W // 7)] = 0.0
        depth[rng.random((H, W)) < 0.02] = 0.0                         # ... and single pixels
        tex = np.stack([np.sin(hit[..., 0] * 5.0) * np.cos(hit[..., 1] * 4.0), np.sin(hit[..., 1] * 7.0 + hit[..., 2]),
                        np.cos(hit[..., 0] * 3.0 - hit[..., 1] * 2.0)], -1)
        image = np.clip(127.5 + 100.0 * tex + rng.normal(0.0, 8.0, (H, W, 3)), 0, 255).astype(np.uint8)
        caps.append(Capture(image, depth.astype(np.float32), K.copy(), c2w))
    return caps[0], caps[1]


def synth_scene(seed, n, H, W, scale=None):
    """A seeded scene of ``n`` >= 3 RGB-D captures of ONE set of planes (those of ``synth_captures``: a tilted background, a
    nearer patch that occludes part of it, holes in the depth) on a ring of poses -> list of ``cotr_amd.data.Capture`` of
    numpy arrays.  Captures 0 ... n - 3 stand on an arc in front of the planes, each a few degrees and a fraction of the depth
    from the next and at its own distance, so their overlaps differ; capture n - 2 stands on the arc but looks AWAY from
    the planes (its depth is all 0 and nothing projects into it: overlap 0 with everything), capture n - 1 looks at the
    planes but has an all-zero depth map (a capture whose depth is missing).
    scale: n factors; capture i is rendered at round(H s_i) x round(W s_i) with K scaled accordingly (same field of view), so
    that many points of a fine capture land on one pixel of a coarse one."""
    from ..data import Capture
    if n < 3:
        raise ValueError('synth_scene needs n >= 3 (an arc, a capture that looks away, a capture without depth)')
    scale = [1.0] * n if scale is None else [float(s) for s in scale]
    if len(scale) != n or min(scale) <= 0:
        raise ValueError('scale must be n positive factors')
    rng = np.random.Generator(np.random.PCG64(seed))
    f = 0.9 * max(H, W)
    K0 = np.array([[f, 0.0, W / 2.0], [0.0, f * 1.02, H / 2.0], [0.0, 0.0, 1.0]])
    planes = [(np.array([0.18, -0.12, 1.0]), 8.0 + rng.uniform(-0.5, 0.5), None),
              (np.array([-0.25, 0.1, 1.0]), 5.0 + rng.uniform(-0.3, 0.3), (rng.uniform(-0.6, 0.2), rng.uniform(-0.4, 0.2), 1.4, 1.1))]

    def rot(ax, ay, az):
        ax, ay, az = np.deg2rad([ax, ay, az])
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        return rz @ ry @ rx

    arc = max(n - 2, 1)
    poses = []                                                         # drawn before anything that depends on H and W: one seed is
    for i in range(n):                                                 # one world and one ring of poses at every resolution
        # the ring: centre (0, 0, 6.5) between the planes, radius about 6.5; the camera at angle a looks at the centre
        a = (min(i, arc - 1) - (arc - 1) / 2.0) * 7.0 + rng.uniform(-1.0, 1.0)
        radius = 6.5 * (1.0 + 0.12 * rng.uniform(-1.0, 1.0))
        c2w = np.eye(4)
        c2w[:3, :3] = rot(*rng.uniform(-1.5, 1.5, 2), 0.0) @ rot(0.0, -a + (180.0 if i == n - 2 else 0.0), rng.uniform(-2.0, 2.0))
        c2w[:3, 3] = np.array([radius * np.sin(np.deg2rad(a)), rng.uniform(-0.2, 0.2), 6.5 - radius * np.cos(np.deg2rad(a))])
        poses.append(c2w)
    caps = []
    for i, c2w in enumerate(poses):
        h, w = max(1, int(round(H * scale[i]))), max(1, int(round(W * scale[i])))
        K = np.diag([w / W, h / H, 1.0]) @ K0
        depth = np.full((h, w), np.inf)
        hit = np.zeros((h, w, 3))
        for normal, offset, rect in planes:
            normal = normal / np.linalg.norm(normal)
            with np.errstate(divide='ignore', invalid='ignore'):
                t, pts = _ray_plane_depth(h, w, K, c2w, normal, offset)
            ok = (t > 0) & (t < depth)
            if rect is not None:
                ok &= (np.abs(pts[..., 0] - rect[0]) < rect[2]) & (np.abs(pts[..., 1] - rect[1]) < rect[3])
            depth = np.where(ok, t, depth)
            hit = np.where(ok[..., None], pts, hit)
        depth = np.where(np.isfinite(depth), depth, 0.0)
        for _ in range(2):                                             # holes: rectangles ...
            h0, w0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            depth[h0:h0 + max(1, h // 9), w0:w0 + max(1, w // 7)] = 0.0
        depth[rng.random((h, w)) < 0.02] = 0.0                         # ... and single pixels
        if i == n - 1:
            depth[:] = 0.0
        tex = np.stack([np.sin(hit[..., 0] * 5.0) * np.cos(hit[..., 1] * 4.0), np.sin(hit[..., 1] * 7.0 + hit[..., 2]),
                        np.cos(hit[..., 0] * 3.0 - hit[..., 1] * 2.0)], -1)
        image = np.clip(127.5 + 100.0 * tex + rng.normal(0.0, 8.0, (h, w, 3)), 0, 255).astype(np.uint8)
        caps.append(Capture(image, depth.astype(np.float32), K, c2w))
    return caps


def state_checksum(sd):
    """float64 (sum, sum of squares) over all tensors, to detect generator drift."""
    s = s2 = 0.0
    for v in sd.values():
        a = np.asarray(v, dtype=np.float64)
        s += float(a.sum())
        s2 += float((a * a).sum())
    return s, s2
