"""Primary-ray tables for Viewport.set_ray_source: pure NumPy builders, no device involved.

Every builder returns ``(origins, directions)``, two float32 arrays of shape (height, width, 3) -- row y as in Viewport.sum_buffer(): row 0 is the top of
the picture -- that go straight into ``viewport.set_ray_source(origins, directions)``.  Directions are unit length here, though the library does not
ask for that; no ray is degenerate (every value finite, no zero direction).

``transform`` is a 4x4 row-major local-to-world matrix as RtCamera::localToWorld holds it (raytracer_amd.transform_from_euler makes one): row 0 points
right, row 1 up, row 2 forward, row 3 is the position.  Anything np.asarray turns into 16 floats is accepted.

``sample_offset = (sx, sy)`` moves the sample inside the pixel, in pixels, x to the right and y up, from the pixel's centre.  For anti-aliasing draw a new
offset per pass and set the table again between passes; each set call ends the batch of passes in flight, so a pass then rides through the launch sequence
alone: measured on the 1080p Sponza-class frame, 6.05 ms per pass with a table set before every pass against 2.32 ms from one table (DESIGN.md section 5,
"Ray source").  ``footprints`` below is the way around that: it turns a builder into a LENS table (Viewport.set_lens_source), which carries every ray's
change per unit of the pass's sample offset -- and a thin lens -- so that one table serves every pass, jittered on the device (DESIGN.md section 5,
"Lens source").
"""
import numpy as np


def _axes(transform):
    m = np.asarray(transform, dtype=np.float64).reshape(4, 4)
    if not np.isfinite(m).all():
        raise ValueError("the transform must be finite")
    return m[0, :3], m[1, :3], m[2, :3], m[3, :3]


def _grid(width, height, sample_offset):
    """unipolar film coordinates of every pixel's sample, u to the right and v up: two (height, width) float64 arrays"""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("width and height must be at least 1")
    sx, sy = float(sample_offset[0]), float(sample_offset[1])
    u = (np.arange(width, dtype=np.float64) + 0.5 + sx) / width
    v = (np.arange(height - 1, -1, -1, dtype=np.float64) + 0.5 + sy) / height   # row y is film row height - 1 - y
    return np.broadcast_to(u[None, :], (height, width)), np.broadcast_to(v[:, None], (height, width))


def _out(origins, directions):
    origins = np.ascontiguousarray(origins, dtype=np.float32)
    directions = np.ascontiguousarray(directions, dtype=np.float32)
    if not (np.isfinite(origins).all() and np.isfinite(directions).all()):
        raise ValueError("the rays are not finite")
    if not (np.einsum("...k,...k->...", directions, directions) > 0.0).all():
        raise ValueError("a direction is zero")
    return origins, directions


def orthographic(width, height, transform, half_width, sample_offset=(0.0, 0.0)):
    """Parallel rays along the transform's forward axis.  The picture is 2 * half_width wide in world units (neighbouring origins lie
    2 * half_width / width apart, in both directions: pixels are square) and centred on the transform's position."""
    right, up, forward, position = _axes(transform)
    half_width = float(half_width)
    if not (half_width > 0.0) or not np.isfinite(half_width):
        raise ValueError("half_width must be positive")
    if not np.dot(forward, forward) > 0.0:
        raise ValueError("the transform's forward axis is zero")
    u, v = _grid(width, height, sample_offset)
    half_height = half_width * int(height) / int(width)
    x = (2.0 * u - 1.0) * half_width
    y = (2.0 * v - 1.0) * half_height
    origins = position + x[..., None] * right + y[..., None] * up
    directions = np.broadcast_to(forward / np.sqrt(np.dot(forward, forward)), origins.shape)
    return _out(origins, directions)


def panorama(width, height, transform, sample_offset=(0.0, 0.0)):
    """An equirectangular view of the full sphere from the transform's position: the columns go once around the up axis (the centre column looks
    forward, the columns to its right turn right), the rows sweep from straight up (row 0) to straight down."""
    right, up, forward, position = _axes(transform)
    u, v = _grid(width, height, sample_offset)
    azimuth = (u - 0.5) * (2.0 * np.pi)
    elevation = (v - 0.5) * np.pi
    ce = np.cos(elevation)
    directions = (ce * np.cos(azimuth))[..., None] * forward + (ce * np.sin(azimuth))[..., None] * right + np.sin(elevation)[..., None] * up
    directions = directions / np.sqrt(np.einsum("...k,...k->...", directions, directions))[..., None]
    return _out(np.broadcast_to(position, directions.shape), directions)


def fisheye(width, height, transform, fov_rad, sample_offset=(0.0, 0.0)):
    """An equidistant fisheye lens: the angle between a ray and the forward axis grows linearly with the sample's distance from the picture's centre and
    reaches fov_rad / 2 on the image circle, the circle inscribed in the picture's shorter side.  fov_rad may exceed pi (up to 2 pi).  Pixels outside the
    image circle repeat the axis ray."""
    right, up, forward, position = _axes(transform)
    fov_rad = float(fov_rad)
    if not (0.0 < fov_rad <= 2.0 * np.pi):
        raise ValueError("fov_rad must be in (0, 2 pi]")
    u, v = _grid(width, height, sample_offset)
    shorter = float(min(int(width), int(height)))
    x = (2.0 * u - 1.0) * (int(width) / shorter)
    y = (2.0 * v - 1.0) * (int(height) / shorter)
    r = np.sqrt(x * x + y * y)
    inside = r <= 1.0
    theta = np.where(inside, r, 0.0) * (0.5 * fov_rad)
    safe = np.where(r > 0.0, r, 1.0)
    st = np.where(inside & (r > 0.0), np.sin(theta) / safe, 0.0)
    directions = np.cos(theta)[..., None] * forward + (st * x)[..., None] * right + (st * y)[..., None] * up
    directions = directions / np.sqrt(np.einsum("...k,...k->...", directions, directions))[..., None]
    return _out(np.broadcast_to(position, directions.shape), directions)


def _radical_inverse2(i):
    i = np.asarray(i, dtype=np.uint64)
    out = np.zeros(i.shape, dtype=np.float64)
    f = 0.5
    while (i > 0).any():
        out += f * (i & np.uint64(1)).astype(np.float64)
        i = i >> np.uint64(1)
        f *= 0.5
    return out


def hemisphere_probe(points, normals, n, sample_offset=(0.0, 0.0), offset=1e-3):
    """n cosine-distributed directions over the hemisphere of each (point, normal) -- what a light probe or a lightmap texel gathers radiance along.  One
    point per row: origins and directions are (len(points), n, 3), a frame n wide and len(points) high, so pixel (j, i) of the rendered frame estimates
    the radiance arriving at point i from its j-th direction and the mean of row i the irradiance over pi.  The directions are a Hammersley set warped by
    the cosine map, the same set around every normal; sample_offset shifts the set (a Cranley-Patterson rotation) for another draw.  The library applies no
    origin offset, so the origins leave the surface by `offset` along the normal."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    n = int(n)
    if points.shape != normals.shape or points.shape[0] < 1 or n < 1:
        raise ValueError("points and normals must be (P, 3) arrays with P >= 1, and n >= 1")
    length = np.sqrt(np.einsum("ik,ik->i", normals, normals))
    if not (length > 0.0).all():
        raise ValueError("a normal is zero")
    nz = normals / length[:, None]
    # an orthonormal basis around each normal (Duff et al. 2017)
    sign = np.where(nz[:, 2] >= 0.0, 1.0, -1.0)
    a = -1.0 / (sign + nz[:, 2])
    b = nz[:, 0] * nz[:, 1] * a
    tx = np.stack([1.0 + sign * nz[:, 0] * nz[:, 0] * a, sign * b, -sign * nz[:, 0]], axis=1)
    ty = np.stack([b, sign + nz[:, 1] * nz[:, 1] * a, -nz[:, 1]], axis=1)
    j = np.arange(n)
    u1 = np.mod((j + 0.5) / n + float(sample_offset[0]), 1.0)
    u2 = np.mod(_radical_inverse2(j) + float(sample_offset[1]), 1.0)
    radius, angle = np.sqrt(u1), 2.0 * np.pi * u2
    lx, ly, lz = radius * np.cos(angle), radius * np.sin(angle), np.sqrt(np.maximum(1.0 - u1, 1e-6))
    directions = lx[None, :, None] * tx[:, None, :] + ly[None, :, None] * ty[:, None, :] + lz[None, :, None] * nz[:, None, :]
    directions = directions / np.sqrt(np.einsum("...k,...k->...", directions, directions))[..., None]
    origins = np.broadcast_to((points + nz * float(offset))[:, None, :], directions.shape)
    return _out(origins, directions)


def _lens_axes(directions, right, up):
    """The lens plane of each direction: U = up x d, normalised, and V = d x U -- a unit pair perpendicular to d that turns into (right, up) where d is the
    transform's forward axis.  Where d is parallel to up (the poles of a panorama: |up x d| < 1e-6) U is the right axis with its part along d removed."""
    d = directions / np.sqrt(np.einsum("...k,...k->...", directions, directions))[..., None]
    u = np.cross(np.broadcast_to(up, d.shape), d)
    length = np.sqrt(np.einsum("...k,...k->...", u, u))
    fallback = right - np.einsum("...k,k->...", d, right)[..., None] * d
    u = np.where((length < 1e-6)[..., None], fallback, u)
    u = u / np.sqrt(np.einsum("...k,...k->...", u, u))[..., None]
    return u, np.cross(d, u)


def footprints(builder, *args, aperture=0.0, focal_distance=1.0, **kw):
    """A lens table for Viewport.set_lens_source from one of the builders above (orthographic, panorama, fisheye): ``footprints(panorama, w, h, transform)``
    returns an (height, width, 32) float32 array of RtLensRay entries.
      stored ray    the builder's ray at sample offset (0, 0)
      derivatives   the builder's own central differences per unit offset, (builder(+1/2) - builder(-1/2)) along x and along y: exact for orthographic,
                    whose rays are linear in the offset; for the angular builders the first-order footprint, whose direction at offset o (before it is
                    normalised) is off the builder's by an angle of second order, below (|o| * theta)^2 with theta the angle between neighbouring pixels
                    (a fisheye pixel whose samples straddle the image circle has no derivative: its footprint is the jump's difference)
      lens axes     orthographic: the transform's right and up axes, normalised; panorama and fisheye: per pixel U = up x d normalised, V = d x U (at a
                    direction parallel to up: U = right with its part along d removed) -- unit length and perpendicular to the stored direction
      aperture, focal_distance   scalars or (height, width) arrays: the lens radius in world units and the distance along the (unit) direction at which the
                    picture is sharp; they take effect when the table is set with lens=True
    ``sample_offset`` is not accepted: the pass's offset is applied on the device."""
    if builder not in (orthographic, panorama, fisheye):
        raise ValueError("footprints takes orthographic, panorama or fisheye")
    if "sample_offset" in kw:
        raise ValueError("a lens table is built at offset 0: the pass's sample offset is applied on the device")
    o0, d0 = builder(*args, sample_offset=(0.0, 0.0), **kw)
    height, width = o0.shape[:2]
    table = np.zeros((height, width, 32), dtype=np.float32)
    table[..., 0:3], table[..., 4:7] = o0, d0
    for axis, (ko, kd) in enumerate(((8, 16), (12, 20))):
        plus = builder(*args, sample_offset=(0.5, 0.0) if axis == 0 else (0.0, 0.5), **kw)
        minus = builder(*args, sample_offset=(-0.5, 0.0) if axis == 0 else (0.0, -0.5), **kw)
        table[..., ko:ko + 3] = plus[0].astype(np.float64) - minus[0].astype(np.float64)
        table[..., kd:kd + 3] = plus[1].astype(np.float64) - minus[1].astype(np.float64)
    transform = kw["transform"] if "transform" in kw else args[2]
    right, up, _, _ = _axes(transform)
    if builder is orthographic:
        lens_u = np.broadcast_to(right / np.sqrt(np.dot(right, right)), d0.shape)
        lens_v = np.broadcast_to(up / np.sqrt(np.dot(up, up)), d0.shape)
    else:
        lens_u, lens_v = _lens_axes(d0.astype(np.float64), right, up)
    table[..., 24:27], table[..., 28:31] = lens_u, lens_v
    table[..., 3] = np.broadcast_to(np.asarray(aperture, dtype=np.float32), (height, width))
    table[..., 7] = np.broadcast_to(np.asarray(focal_distance, dtype=np.float32), (height, width))
    if not np.isfinite(table).all():
        raise ValueError("the lens table is not finite")
    return table
