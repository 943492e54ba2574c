"""Deterministic synthetic KITTI-shaped stereo data (no dataset, no network).

Scene: a textured corridor (ground plane, two side walls, a ceiling and a far end wall) seen by a
rectified stereo rig with the KITTI-00 intrinsics the reference hard-codes
(ref: include/image_processing_global.h:35-36, run_odometry_kitti_offline.cpp:38-41).
Images are rendered per pixel (ray/plane intersection + bilinear lookup in a tileable multi-octave
value-noise texture), then quantised to u8 and cast to fp32 — the same value range and granularity as
the reference's imread(GRAYSCALE) -> convertTo(CV_32F) (ref: run_odometry_kitti_offline.cpp:334-359).

Coordinates: x right, y down, z forward. Poses are camera-to-world 4x4 (float64).
"""
import numpy as np

KITTI_F = 718.856
KITTI_CX = 607.1928
KITTI_CY = 185.2157
KITTI_BASELINE = 386.1448 / 718.856
KITTI_ROWS, KITTI_COLS = 376, 1241
TUM_F, TUM_CX, TUM_CY = 525.0, 319.5, 239.5   # TUM RGB-D-shaped sensor (640 x 480)
TUM_ROWS, TUM_COLS = 480, 640


def _value_noise(rng, size, octaves, first_cell):
    """Tileable multi-octave value noise in [0,1], `size` x `size` (bilinear-interpolated lattices)."""
    tex = np.zeros((size, size), np.float64)
    amp, tot, cell = 1.0, 0.0, first_cell
    ii = np.arange(size)
    for _ in range(octaves):
        n = size // cell
        lat = rng.random((n, n))
        g = ii / cell
        i0 = np.floor(g).astype(np.int64) % n
        i1 = (i0 + 1) % n
        f = g - np.floor(g)
        f = f * f * (3 - 2 * f)
        a = lat[np.ix_(i0, i0)] * (1 - f)[None, :] + lat[np.ix_(i0, i1)] * f[None, :]
        b = lat[np.ix_(i1, i0)] * (1 - f)[None, :] + lat[np.ix_(i1, i1)] * f[None, :]
        tex += amp * (a * (1 - f)[:, None] + b * f[:, None])
        tot += amp
        amp *= 0.6
        cell = max(cell // 2, 2)
    return tex / tot


class Scene:
    """Corridor of textured planes. texels_per_m controls texture scale."""

    def __init__(self, seed=0, half_width=(4.0, 5.0), cam_height=1.65, ceil_height=3.0, end_z=600.0,
                 tex_size=1024, texels_per_m=60.0, tile_texels=(11, 29, 67), contrast=(1.0, 1.0, 1.0, 1.0, 1.0),
                 spectrum=None, sigma=40.0, tile_amp=0.0, ribs=None):
        rng = np.random.default_rng(0x0D0E77E7 + 1000 * seed)
        self.tex = []
        for _ in range(5 if spectrum is not None else 0):
            # natural-image statistics: amplitude spectrum ~ 1 / f^spectrum (random phases, tileable by construction), so
            # that coarse pyramid levels carry most of the contrast — what makes coarse-to-fine alignment of real images work
            fy = np.fft.fftfreq(tex_size)[:, None]
            fx = np.fft.rfftfreq(tex_size)[None, :]
            f = np.sqrt(fx * fx + fy * fy)
            f[0, 0] = 1.0
            amp = 1.0 / f ** spectrum
            amp[0, 0] = 0.0
            ph = rng.uniform(0.0, 2.0 * np.pi, amp.shape)
            t = np.fft.irfft2(amp * np.exp(1j * ph), s=(tex_size, tex_size))
            t = (t - t.mean()) / t.std()
            tiles = np.zeros_like(t)
            if tile_amp > 0.0:
                ii = np.arange(tex_size)
                for s_ in tile_texels:
                    nc = tex_size // s_ + 1
                    cells = rng.uniform(-1.0, 1.0, (nc, nc))
                    tiles += cells[np.ix_(ii // s_, ii // s_)]
                tiles /= np.sqrt(len(tile_texels))
            self.tex.append(np.clip(128.0 + sigma * t + tile_amp * tiles, 0.0, 255.0))
        for _ in range(5 if spectrum is None else 0):  # smooth value noise + random-brightness tiles (sparse strong edges)
            t = _value_noise(rng, tex_size, 6, 128)
            t = (t - t.mean()) / t.std()
            tiles = np.zeros_like(t)
            ii = np.arange(tex_size)
            for s_ in tile_texels:  # incommensurate tile sizes: irregular edge layout, no strict period
                nc = tex_size // s_ + 1
                cells = rng.uniform(-1.0, 1.0, (nc, nc))
                tiles += cells[np.ix_(ii // s_, ii // s_)]
            tiles /= np.sqrt(len(tile_texels))
            self.tex.append(np.clip(128.0 + 22.0 * t + 50.0 * tiles, 0.0, 255.0))
        self.tpm = texels_per_m
        # ribs = (spacing, half_opening, opening_height): fronto-parallel frames across the corridor every `spacing` metres (z = k *
        # spacing), each with a doorway |x| < half_opening below `opening_height` above the ground that the camera drives through —
        # tunnel ribs / gantries: textured structure AHEAD of the camera at every depth, near the focus of expansion
        self.ribs = ribs
        self.cam_height = cam_height
        self.contrast = contrast   # per plane (ground, left wall, right wall, ceiling / sky, end wall): grey = 128 + c * (tex - 128)
        # planes: (normal n, offset h) with n . X = h; texture axes (a, b) index world coords
        self.planes = [
            (np.array([0.0, 1.0, 0.0]), cam_height, (0, 2)),        # ground  y = +h
            (np.array([1.0, 0.0, 0.0]), -half_width[0], (2, 1)),    # left wall
            (np.array([1.0, 0.0, 0.0]), half_width[1], (2, 1)),     # right wall
            (np.array([0.0, 1.0, 0.0]), -ceil_height, (0, 2)),      # ceiling
            (np.array([0.0, 0.0, 1.0]), end_z, (0, 1)),             # end wall
        ]

    def _sample(self, k, u, v):
        tex = self.tex[k]
        n = tex.shape[0]
        u = u * self.tpm
        v = v * self.tpm
        u0 = np.floor(u)
        v0 = np.floor(v)
        fu = u - u0
        fv = v - v0
        u0 = u0.astype(np.int64) % n
        v0 = v0.astype(np.int64) % n
        u1 = (u0 + 1) % n
        v1 = (v0 + 1) % n
        return (tex[v0, u0] * (1 - fu) * (1 - fv) + tex[v0, u1] * fu * (1 - fv) +
                tex[v1, u0] * (1 - fu) * fv + tex[v1, u1] * fu * fv)

    def render(self, pose_c2w, rows=KITTI_ROWS, cols=KITTI_COLS, f=KITTI_F, cx=KITTI_CX, cy=KITTI_CY,
               x_offset=0.0):
        """Returns (image fp32 u8-quantised, depth Z fp64). x_offset shifts the camera along its own x
        axis (the right camera of the rig is x_offset = +baseline)."""
        R = pose_c2w[:3, :3]
        t = pose_c2w[:3, 3] + R[:, 0] * x_offset
        xs = (np.arange(cols) - cx) / f
        ys = (np.arange(rows) - cy) / f
        dx, dy = np.meshgrid(xs, ys)
        dirs = np.stack([dx, dy, np.ones_like(dx)], -1) @ R.T     # world-frame ray directions (z_c = 1)
        best = np.full((rows, cols), np.inf)
        img = np.zeros((rows, cols))
        for k, (n, h, (a, b)) in enumerate(self.planes):
            den = dirs @ n
            num = h - n @ t
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(np.abs(den) > 1e-12, num / den, np.inf)
            hit = (s > 1e-3) & (s < best)
            if not hit.any():
                continue
            P = t[None, :] + dirs[hit] * s[hit][:, None]
            img[hit] = 128.0 + self.contrast[k] * (self._sample(k, P[:, a], P[:, b]) - 128.0)
            best[hit] = s[hit]
        if self.ribs is not None:
            spacing, half_open, open_h = self.ribs
            k0 = int(np.floor(t[2] / spacing)) + 1
            dz = dirs[..., 2]
            for k in range(k0, k0 + 14):                      # nearest first; farther ribs only where nothing nearer was hit
                with np.errstate(divide="ignore", invalid="ignore"):
                    sk = np.where(dz > 1e-9, (k * spacing - t[2]) / dz, np.inf)
                cand = (sk > 1e-3) & (sk < best)
                if not cand.any():
                    continue
                P = t[None, :] + dirs[cand] * sk[cand][:, None]
                solid = (np.abs(P[:, 0]) > half_open) | (P[:, 1] < self.cam_height - open_h)     # y is down: above the doorway
                idx = np.flatnonzero(cand.ravel())[solid]
                if idx.size == 0:
                    continue
                Ps = P[solid]
                val = 128.0 + self.contrast[4] * (self._sample(4, Ps[:, 0] + 3.7 * k, Ps[:, 1] + 1.3 * k) - 128.0)
                img.ravel()[idx] = val
                best.ravel()[idx] = sk.ravel()[idx]
        img = np.clip(np.rint(img), 0, 255).astype(np.float32)
        return img, best


# Named drives: scene + motion. "corridor" is the drive of rounds 1-2 (everything within 5-30 m of the camera, 0.3-0.6 m per
# frame): on it the reference's keyframe policy loses track at every keyframe switch. The others are
# candidates evaluated with tools/drive_search.py.
DRIVES = {
    "corridor": dict(scene={}, fwd_range=(0.3, 0.6), max_offset=1.0),
    # bench.py's workload since round 3. Same corridor and motion; the textures have the amplitude spectrum of natural images
    # (~ 1 / f^1.55, sigma 80 grey levels before clipping) instead of white-ish value noise + hard-edged tiles. Coarse pyramid levels
    # then carry most of the contrast, the basin of the level-3 alignment is wide enough for the first Solve after a keyframe switch
    # (which starts ~3.6 m off: the reference resets to the pose relative to the OLD keyframe, ref: run_odometry_kitti_offline.cpp:
    # 261-262) to converge in 21 of 25 switches over 200 frames; the tracker stays within centimetres of the ground truth on 195 of
    # 199 frames (tools/drive_search.py natural 200). Found by scanning spectrum x contrast x speed x corridor width with the oracle.
    "natural": dict(scene=dict(spectrum=1.55, sigma=80.0), fwd_range=(0.3, 0.6), max_offset=1.0),
    # bench.py's saturated_keyframe leg (round 4): a flatter spectrum (~ 1 / f^1.2) puts enough fine texture into every 38 x 23 block
    # for the point selection to hit its cap of 80 per block (ref: src/depth_estimate.cpp:300-304,333-339): 39 805 of 40 960 slots
    # selected, ~28 700 valid inverse depths on level 0 of a keyframe (the natural drive: 18 037 / 13 643) — what a richly textured
    # real frame does to the pose LM's finest level.
    "dense": dict(scene=dict(spectrum=1.2, sigma=80.0), fwd_range=(0.3, 0.6), max_offset=1.0),
}


def trajectory(n_frames, seed=0, fwd_range=(0.3, 0.6), max_offset=1.0, yaw_deg=1.5, yaw_total_deg=6.0):
    """Camera-to-world poses: forward fwd_range m/frame, yaw <= 1.5 deg, pitch/roll <= 0.2 deg per frame."""
    rng = np.random.default_rng(0x0D0E77E7 + 1000 * seed + 17)
    poses = [np.eye(4)]
    yaw_total = 0.0
    for _ in range(1, n_frames):
        fwd = rng.uniform(*fwd_range)
        yaw = np.deg2rad(rng.uniform(-yaw_deg, yaw_deg))
        if abs(yaw_total + yaw) > np.deg2rad(yaw_total_deg):  # stay inside the corridor
            yaw = -yaw
        pitch = np.deg2rad(rng.uniform(-0.2, 0.2))
        roll = np.deg2rad(rng.uniform(-0.2, 0.2))
        # long sequences: steer back towards the corridor axis once the camera has drifted (same random draws, so
        # short sequences — which never drift this far — are unchanged)
        cur = poses[-1]
        if abs(cur[0, 3]) > max_offset and np.sign(yaw) == np.sign(cur[0, 3]) and np.sign(cur[0, 2]) == np.sign(cur[0, 3]):
            yaw = -yaw                                   # heading away from the axis: turn the other way
        if abs(cur[1, 3]) > 0.3 and np.sign(cur[1, 2]) == np.sign(cur[1, 3]) and np.sign(-pitch) == np.sign(cur[1, 3]):
            pitch = -pitch
        yaw_total += yaw
        cy_, sy_ = np.cos(yaw), np.sin(yaw)
        cp, sp = np.cos(pitch), np.sin(pitch)
        cr, sr = np.cos(roll), np.sin(roll)
        Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
        Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        d = np.eye(4)
        d[:3, :3] = Ry @ Rx @ Rz
        d[:3, 3] = [rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), fwd]
        poses.append(poses[-1] @ d)
    return poses


def drive_scene(drive, seed):
    return Scene(seed, **DRIVES[drive]["scene"])


def drive_trajectory(drive, n_frames, seed):
    return trajectory(n_frames, seed, **{k: v for k, v in DRIVES[drive].items() if k != "scene"})


def make_sequence(n_frames, seed=0, rows=KITTI_ROWS, cols=KITTI_COLS, f=KITTI_F, cx=KITTI_CX, cy=KITTI_CY,
                  baseline=KITTI_BASELINE, with_depth=False, drive="corridor"):
    """Returns dict(left=[...], right=[...], poses=[c2w...], depth=[...] optional)."""
    scene = drive_scene(drive, seed)
    poses = drive_trajectory(drive, n_frames, seed)
    out = dict(left=[], right=[], poses=poses, depth=[])
    for T in poses:
        L, Z = scene.render(T, rows, cols, f, cx, cy, 0.0)
        Rimg, _ = scene.render(T, rows, cols, f, cx, cy, baseline)
        out["left"].append(L)
        out["right"].append(Rimg)
        if with_depth:
            out["depth"].append(Z)
    return out


def sensor_depth(Z, depth_scale=1000.0, max_range=30.0):
    """An RGB-D sensor's uint16 depth frame of the z-depth Z (metres): round(Z * depth_scale) where Z <= max_range and the value fits
    in 16 bits, else 0 (no reading)."""
    raw = np.rint(np.asarray(Z, np.float64) * depth_scale)
    ok = np.isfinite(raw) & (np.asarray(Z) <= max_range) & (raw <= 65535)
    return np.where(ok, raw, 0).astype(np.uint16)


KINECT_AXIAL_NOISE = (0.0012, 0.0019, 0.4)   # sigma(z) = 1.2 mm + 1.9 mm (z - 0.4 m)^2: the published Kinect axial noise model


def sensor_noise(Z, rng, noise=KINECT_AXIAL_NOISE, max_range=30.0):
    """Z (metres) with a depth sensor's axial noise added, in front of sensor_depth: Gaussian, zero mean, standard deviation
    sigma(z) = a + b (z - z0)^2 metres with noise = (a, b, z0). rng: a numpy Generator (one standard normal per pixel is drawn,
    whatever Z holds). Pixels beyond max_range (where sensor_depth has no reading, and the model's sigma would be tens of metres)
    and pixels that are not finite stay as they are; a noisy depth below 0 is 0, which sensor_depth turns into "no reading"."""
    Z = np.asarray(Z, np.float64)
    a, b, z0 = noise
    n = rng.standard_normal(Z.shape)
    keep = ~np.isfinite(Z) | (Z > max_range)
    Zs = np.where(keep, 0.0, Z)
    return np.where(keep, Z, np.maximum(Zs + (a + b * (Zs - z0) ** 2) * n, 0.0))


def depth_noise_rng(depth_noise, k):
    """The generator of frame k's noise: depth_noise = seed, or (seed, (a, b, z0)). One generator per frame, so that a frame's
    noise does not depend on which other frames were rendered."""
    seed, noise = depth_noise if isinstance(depth_noise, tuple) else (depth_noise, KINECT_AXIAL_NOISE)
    return np.random.default_rng([0x0D0E77E7, int(seed), int(k)]), noise


def make_rgbd_sequence(n_frames, seed=0, drive="natural", fwd_range=(0.1, 0.2), depth_scale=1000.0, max_range=30.0, rows=TUM_ROWS,
                       cols=TUM_COLS, f=TUM_F, cx=TUM_CX, cy=TUM_CY, depth_noise=None):
    """An RGB-D drive: grey frames of the named drive's scene (Scene.render) and the sensor's depth frames (sensor_depth), along the
    drive's trajectory with fwd_range metres per frame. TUM-shaped by default. depth_noise: None, a noise seed, or (seed, (a, b,
    z0)): sensor_noise on every frame's Z in front of sensor_depth. Returns dict(gray=[...], depth=[uint16 ...],
    poses=[c2w ...], K=dict(f0, cx0, cy0), depth_scale, max_range)."""
    scene = drive_scene(drive, seed)
    kw = {k: v for k, v in DRIVES[drive].items() if k not in ("scene", "fwd_range")}
    poses = trajectory(n_frames, seed, fwd_range=fwd_range, **kw)
    out = dict(gray=[], depth=[], poses=poses, K=dict(f0=f, cx0=cx, cy0=cy), depth_scale=depth_scale, max_range=max_range)
    for k, T in enumerate(poses):
        img, Z = scene.render(T, rows, cols, f, cx, cy, 0.0)
        if depth_noise is not None:
            Z = sensor_noise(Z, *depth_noise_rng(depth_noise, k), max_range=max_range)
        out["gray"].append(img)
        out["depth"].append(sensor_depth(Z, depth_scale, max_range))
    return out


def rig_extrinsic(t_m=(0.0, 0.0, 0.0), rot_rad=(0.0, 0.0, 0.0)):
    """colour_from_depth as a 4x4: P_c = R P_d + t with R = Rz Ry Rx of the angles about x, y, z (radians), t in metres."""
    rx, ry, rz = rot_rad
    cx_, sx_, cy_, sy_, cz_, sz_ = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rz = np.array([[cz_, -sz_, 0], [sz_, cz_, 0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = Rz @ Ry @ Rx
    E[:3, 3] = t_m
    return E


def colour_from_gray(gray, channels=3, bgr=False, tint_seed=None):
    """An interleaved uint8 colour frame of a grey image (values 0..255): the grey value in R, G and B, or — with tint_seed — a
    seeded gain and offset per channel so that the three differ; a fourth channel holds seeded noise (a front end ignores it)."""
    g = np.asarray(gray, np.float64)
    if tint_seed is None:
        rgb = [g, g, g]
        rng = np.random.default_rng(0x7157)
    else:
        rng = np.random.default_rng(0x7157 + tint_seed)
        rgb = [g * rng.uniform(0.6, 1.2) + rng.uniform(-20.0, 20.0) for _ in range(3)]
    planes = [np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (rgb[::-1] if bgr else rgb)]
    if channels == 4:
        planes.append(rng.integers(0, 256, g.shape).astype(np.uint8))
    return np.ascontiguousarray(np.stack(planes, -1))


def make_raw_rgbd_sequence(n_frames, seed=0, drive="natural", fwd_range=(0.1, 0.2), depth_scale=1000.0, max_range=30.0, rows=TUM_ROWS,
                           cols=TUM_COLS, f=TUM_F, cx=TUM_CX, cy=TUM_CY, depth_size=None, depth_f=None, depth_c=None,
                           colour_from_depth=None, channels=3, bgr=False, tint_seed=None, frames=None, depth_noise=None):
    """What an RGB-D sensor delivers along the drive of make_rgbd_sequence: per frame an interleaved uint8 colour frame rendered at
    the colour camera (rows x cols, f, cx, cy; colour_from_gray of the grey rendering) and a uint16 depth frame rendered AT THE DEPTH
    IMAGER: depth_size = (rows, cols), focal length depth_f, principal point depth_c = (cx, cy) (default: the image centre), pose
    T @ colour_from_depth (4x4, P_c = R P_d + t; default identity). Defaults make the depth imager the colour camera.
    frames: the frame indices to render (default all). depth_noise: as make_rgbd_sequence, on the depth imager's Z (depth_gt stays
    clean). Returns dict(colour=[...], raw_depth=[...], gray=[fp32 grey renderings],
    depth_gt=[the registered ground truth: sensor_depth of the colour camera's Z], frames=[indices], poses (all n_frames), K,
    depth_K=(fx, fy, cx, cy), colour_from_depth, depth_scale, max_range)."""
    scene = drive_scene(drive, seed)
    kw = {k: v for k, v in DRIVES[drive].items() if k not in ("scene", "fwd_range")}
    poses = trajectory(n_frames, seed, fwd_range=fwd_range, **kw)
    drows, dcols = (rows, cols) if depth_size is None else depth_size
    fd = f if depth_f is None else depth_f
    if depth_c is not None:
        cxd, cyd = depth_c
    elif depth_size is None and depth_f is None:
        cxd, cyd = cx, cy
    else:
        cxd, cyd = (dcols - 1) / 2.0, (drows - 1) / 2.0
    E = np.eye(4) if colour_from_depth is None else np.asarray(colour_from_depth, np.float64)
    idx = list(range(n_frames)) if frames is None else list(frames)
    out = dict(colour=[], raw_depth=[], gray=[], depth_gt=[], frames=idx, poses=poses, K=dict(f0=f, cx0=cx, cy0=cy),
               depth_K=(fd, fd, cxd, cyd), colour_from_depth=E, depth_scale=depth_scale, max_range=max_range)
    for k in idx:
        T = poses[k]
        img, Z = scene.render(T, rows, cols, f, cx, cy, 0.0)
        _, Zd = scene.render(T @ E, drows, dcols, fd, cxd, cyd, 0.0)
        if depth_noise is not None:
            Zd = sensor_noise(Zd, *depth_noise_rng(depth_noise, k), max_range=max_range)
        out["gray"].append(img)
        out["colour"].append(colour_from_gray(img, channels, bgr, tint_seed))
        out["raw_depth"].append(sensor_depth(Zd, depth_scale, max_range))
        out["depth_gt"].append(sensor_depth(Z, depth_scale, max_range))
    return out


def semi_dense_inverse_depth(Z, left, grad_th=12.0, max_depth=30.0, stride_keep=1.0, seed=0):
    """Ground-truth inverse-depth map restricted to high-gradient pixels (semi-dense), 0 elsewhere —
    a stand-in for DepthEstimator output when a test needs a known-good keyframe depth."""
    gx = np.zeros_like(left)
    gy = np.zeros_like(left)
    gx[:, 1:-1] = 0.5 * (left[:, 2:] - left[:, :-2])
    gy[1:-1, :] = 0.5 * (left[2:, :] - left[:-2, :])
    mask = (np.hypot(gx, gy) > grad_th) & (Z < max_depth)
    if stride_keep < 1.0:
        rng = np.random.default_rng(seed)
        mask &= rng.random(mask.shape) < stride_keep
    inv = np.zeros(Z.shape, np.float32)
    inv[mask] = (1.0 / Z[mask]).astype(np.float32)
    return inv


def integer_disparity_pair(seed=0, rows=KITTI_ROWS, cols=KITTI_COLS, band=24, dmin=3, dmax=96):
    """Known-answer stereo pair: right[y, x - d(y)] = left[y, x] with an integer disparity d per
    horizontal band. Away from band edges (>= 3 rows) the 8-tap SSD at the true match is exactly 0."""
    rng = np.random.default_rng(0x0D0E77E7 + 7919 * seed)
    n = 2048
    tex = _value_noise(rng, n, 7, 64)
    tex = 25.0 * (tex - tex.mean()) / tex.std()
    ii = np.arange(n)
    for s_ in (7, 17, 41):  # random-brightness tiles: sparse strong edges so the block-median selection fires
        cells = rng.uniform(-1.0, 1.0, (n // s_ + 1, n // s_ + 1))
        tex += 28.0 * cells[np.ix_(ii // s_, ii // s_)]
    left = np.clip(np.rint(128.0 + tex[:rows, :cols]), 0, 255).astype(np.float32)
    fill = np.clip(np.rint(128.0 + tex[rows:2 * rows, :cols]), 0, 255).astype(np.float32)
    right = fill.copy()
    disp = np.zeros((rows, cols), np.int32)
    nb = (rows + band - 1) // band
    ds = rng.integers(dmin, dmax + 1, nb)
    for b in range(nb):
        d = int(ds[b])
        y0, y1 = b * band, min(rows, (b + 1) * band)
        right[y0:y1, :cols - d] = left[y0:y1, d:]
        disp[y0:y1, :] = d
    return left, right, disp
