"""Ray lists for Renderer.trace_rays (mm_trace_rays): the record packer and two
cameras the pinhole calls cannot be -- a 360-degree equirectangular view and
an orthographic one.  The camera helpers are plain float32 torch arithmetic:
their rays are what they return, with no bit promise against another
implementation; trace_rays' result for a given record is exact."""
from __future__ import annotations

import math


def pack_rays(origins, dirs, keys):
    """(n, 8) float32 ray records (ox, oy, oz, key, dx, dy, dz, 0) from (n, 3)
    float32 origins and directions and n integer RNG keys, on the origins'
    device.  The key's 32 BITS go into word 3 (no float conversion): the word
    reads back as the key through .view(torch.int32)."""
    import torch

    origins = torch.as_tensor(origins, dtype=torch.float32)
    dirs = torch.as_tensor(dirs, dtype=torch.float32, device=origins.device)
    if origins.ndim != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise ValueError("origins and dirs must both be (n, 3)")
    n = origins.shape[0]
    keys = torch.as_tensor(keys, device=origins.device)
    if keys.is_floating_point() or keys.numel() != n:
        raise ValueError(f"keys must be {n} integers")
    bits = keys.reshape(n).to(torch.int64) & 0xFFFFFFFF  # the low 32 bits, then as int32 holds them
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=origins.device)
    rays[:, 0:3] = origins
    rays[:, 4:7] = dirs
    rays.view(torch.int32)[:, 3] = bits
    return rays


def rotate(quat, v):
    """The camera's rotation of the (..., 3) vectors v: q^-1 v q for the unit
    quaternion quat = (x, y, z, w), the product the pinhole's primary direction
    goes through (src/shaders.metal:281-284)."""
    import torch

    q = torch.as_tensor(quat, dtype=torch.float32, device=v.device).reshape(4)
    qv, qw = (-q[:3]).expand_as(v), q[3]
    t = 2.0 * torch.linalg.cross(qv, v, dim=-1)
    return v + qw * t + torch.linalg.cross(qv, t, dim=-1)


def _pixel_grid(w, h, device):
    import torch

    y, x = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
    return x.reshape(-1), y.reshape(-1)


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def equirect_rays(center, quat, w: int, h: int, device="cuda"):
    """The (w*h, 8) records of a w x h equirectangular panorama from `center`:
    pixel (x, y), row-major, looks along longitude ((x + 0.5)/w - 0.5) * 2 pi
    and latitude ((y + 0.5)/h - 0.5) * pi of the camera frame the pinhole uses
    (+z forward, +x right, +y down, rotated by `quat`), so the image's centre
    is the pinhole's centre.  Unit directions; key y*w + x."""
    import torch

    x, y = _pixel_grid(w, h, device)
    lon = ((x.to(torch.float32) + 0.5) / w - 0.5) * (2.0 * math.pi)
    lat = ((y.to(torch.float32) + 0.5) / h - 0.5) * math.pi
    d = torch.stack([torch.sin(lon) * torch.cos(lat), torch.sin(lat), torch.cos(lon) * torch.cos(lat)], dim=1)
    d = _unit(rotate(quat, d))
    o = torch.as_tensor(center, dtype=torch.float32, device=d.device).reshape(1, 3).expand(w * h, 3)
    return pack_rays(o, d, y * w + x)


def ortho_rays(origin, right, down, forward, w: int, h: int, device="cuda"):
    """The (w*h, 8) records of a w x h orthographic view: pixel (x, y),
    row-major, starts at origin + ((x + 0.5)/w) * right + ((y + 0.5)/h) * down
    -- `origin` is the image's top-left corner, `right` and `down` span it --
    and looks along `forward`, normalised.  Key y*w + x."""
    import torch

    x, y = _pixel_grid(w, h, device)
    vec = [torch.as_tensor(v, dtype=torch.float32, device=x.device).reshape(1, 3) for v in (origin, right, down, forward)]
    o = vec[0] + ((x.to(torch.float32) + 0.5) / w)[:, None] * vec[1] + ((y.to(torch.float32) + 0.5) / h)[:, None] * vec[2]
    d = _unit(vec[3]).expand(w * h, 3)
    return pack_rays(o, d, y * w + x)
