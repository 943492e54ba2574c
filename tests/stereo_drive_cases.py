"""A stereo drive and a matcher's life over many pairs as code, shared by tests/test_stereo_drive_cpu.py and
tests/test_gpu_stereo_drive.py (INTEGRATION.md sections 3.15 to 3.17; DESIGN.md sections 9.16 to 9.18). Nothing here loads the GPU
library, and no model is written here: every link is the model its own tests already hold the kernels to.

  match      stereo_depth_cases.stereo_model (box) or stereo_sgm_cases.sgm_model (semi-global)
  filter     speckle_cases.speckle_model on the q frame, speckle_cases.apply_keep on the q frame and the depth frame
  the loop   volume_follow_track_cases.drive_model on the filtered model depth: ray-cast, alignment, follow step, stores, fusion

The drive: volume_follow_track_cases' ribbed corridor and trajectory, 8 poses at 120 x 160, each rendered twice (the right camera
BASELINE to the right), one frame blind (both images constant). stereo_drive(front) keeps every frame's pair and model outputs;
stereo_drive_model(front) is the closed loop on them, every frame started from the pose the frame before it returned.

The sequence: sequence_steps() is the life of ONE matcher of 40 x 120: a step is (pair, mode, speckle, output frame), and between
two steps the mode, the filter and the output frame change as a caller may change them. step_model(i) is the model of step i ALONE:
what a matcher that carries nothing over from the steps before must give."""
import functools
import time

import numpy as np

import speckle_cases as sc
import stereo_depth_cases as sdc
import stereo_sgm_cases as sgc
import volume_follow_track_cases as F
from test_volume_cpu import params as volume_params
from test_volume_icp_cpu import RIBBED_SCENE, SMALL, icp, small_K

f32 = np.float32
FRONTS = ("box", "sgm")

# ---- the drive --------------------------------------------------------------------------------------------------------------------
BASELINE = 0.5
N_FRAMES = 8
BLIND = (4,)
BLIND_GREY = 90.0
DRIVE_SPECKLE = (16, 100)          # max_diff in sixteenths of a pixel, min_size


def drive_params():
    """The matcher of the drive: candidates 4 .. 51 (0.8 m .. 10 m at this focal length and baseline), readings beyond 5 m rejected:
    the volume's max_depth."""
    f = small_K()[0]
    return sdc.params(dmin=4, dmax=51, A=2, uniq=10, lr_max=1, fx=f, baseline=BASELINE, depth_scale=1000.0, max_raw=5000)


def front_model(mode, L, R, p):
    """dict(depth, q, stats, S) of one pair from the front end's model; mode: None (the box matcher, S None) or the semi-global
    mode's dict(p1, p2, paths)."""
    if mode is None:
        depth, q, stats = sdc.stereo_model(L, R, p)
        return dict(depth=depth, q=q, stats=stats, S=None)
    depth, q, stats, S = sgc.sgm_model(L, R, p, mode)
    return dict(depth=depth, q=q, stats=stats, S=S)


def filtered(m, speckle):
    """m with the speckle filter behind it: M (the filter's model on the q frame, None while it is off) and what a run leaves in the
    depth frame and in the q frame, fdepth and fq."""
    M = sc.speckle_model(m["q"], *speckle) if speckle else None
    out = dict(m, M=M, fdepth=sc.apply_keep(m["depth"], M) if M else m["depth"], fq=sc.apply_keep(m["q"], M) if M else m["q"])
    for key in ("depth", "q", "S", "fdepth", "fq"):
        if out[key] is not None:
            out[key].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stereo_drive(front):
    """A drive dict for volume_follow_track_cases.drive_model (depth = the filtered model frames) with the stereo side of it: left,
    right (fp32 images), mp (the matcher's parameters), sg (the mode, None for "box"), speckle, frames[k] = filtered(front_model) and
    seconds, the time the front end's models took."""
    from odometry_amd import synth
    assert front in FRONTS
    scene = synth.Scene(0, **RIBBED_SCENE)
    poses = list(synth.trajectory(N_FRAMES, 0, fwd_range=(0.1, 0.2), max_offset=1.0))
    f, cx, cy = small_K()
    left = [np.asarray(scene.render(T, SMALL[0], SMALL[1], f, cx, cy, 0.0)[0], f32) for T in poses]
    right = [np.asarray(scene.render(T, SMALL[0], SMALL[1], f, cx, cy, BASELINE)[0], f32) for T in poses]
    for k in BLIND:
        left[k], right[k] = np.full(SMALL, BLIND_GREY, f32), np.full(SMALL, BLIND_GREY, f32)
    for a in left + right:
        a.setflags(write=False)
    mp, sg = drive_params(), sgc.sgm() if front == "sgm" else None
    t = time.time()
    frames = [filtered(front_model(sg, l, r, mp), DRIVE_SPECKLE) for l, r in zip(left, right)]
    seconds = time.time() - t
    p = volume_params((f, cx, cy), 1000.0, SMALL, **F.WINDOW)
    return dict(name=f"stereo {front}", depth=[m["fdepth"] for m in frames], poses=[np.asarray(T, f32) for T in poses], p=p, follow=dict(F.FOLLOW),
                blind=BLIND, ic=icp(p=p, min_eig_ratio=0.0), checkpoints=(), left=left, right=right, mp=mp, sg=sg, speckle=DRIVE_SPECKLE,
                frames=frames, seconds=seconds)


@functools.lru_cache(maxsize=None)
def stereo_drive_model(front):
    """volume_follow_track_cases.drive_model (the device's sums, the host build's step, the point store) on the drive's filtered
    model depth, once per process, and the seconds it took."""
    c = stereo_drive(front)
    t = time.time()
    m = F.drive_model(c, spill=True)
    m["seconds"] = time.time() - t
    return m


# ---- the sequence -----------------------------------------------------------------------------------------------------------------
SEQ_SIZE = (40, 120)
MODES = dict(box=None, sgm8=sgc.sgm(), sgm4=sgc.sgm(p1=7, p2=900, paths=4))
SPECKLES = (None, (16, 60), (4, 20))
FLAT_GREY = 90.0


def sequence_params():
    return sdc.params(dmin=1, dmax=24)


@functools.lru_cache(maxsize=None)
def sequence_pairs():
    """name -> (L, R), all SEQ_SIZE fp32 and read-only. Synthetic pairs match almost everywhere, so what tells one step's q frame
    from the next one's is WHERE each pair cannot be matched: the left strip of a shift (17 or 20 columns wide), the band an
    occluder hides from the right image (8 or 18 columns, mid-frame), nearly everything for a period below dmax under the box
    matcher and for the exchanged pair (whose disparities are negative). "shift 5" and "constant" have no such region to speak of:
    tests/test_stereo_drive_cpu.py says what that means for the steps next to them."""
    flat = np.full(SEQ_SIZE, FLAT_GREY, f32)
    occ = sdc.occluding_step(43, SEQ_SIZE)
    out = {"shift 5": sdc.shifted_pair(41, SEQ_SIZE, 5), "shift 17": sdc.shifted_pair(42, SEQ_SIZE, 17), "occluding step 4/12": occ,
           "occluding step 2/20": sdc.occluding_step(43, SEQ_SIZE, 2, 20), "non-finite": sdc.non_finite_pair(44, SEQ_SIZE, 20),
           "periodic": sdc.periodic_pair(45, SEQ_SIZE, 11, 3), "constant": (flat, flat.copy()), "exchanged": (occ[1], occ[0])}
    out = {name: tuple(np.ascontiguousarray(a, f32) for a in pair[:2]) for name, pair in out.items()}
    for pair in out.values():
        for a in pair:
            assert a.shape == SEQ_SIZE
            a.setflags(write=False)
    return out


TEXTURED = ("shift 5", "shift 17", "occluding step 4/12", "occluding step 2/20", "non-finite", "periodic")


def sequence_steps():
    """[(pair, mode, speckle, output)]: pair a name of sequence_pairs(), mode a name of MODES, speckle one of SPECKLES, output
    "internal" or "caller" (a guarded frame of the caller's). Ordered so that every mode follows every other one, the semi-global
    mode is re-parametrised in place both ways (the volumes stay), the filter goes on, is re-parametrised and goes off, and the
    constant and the exchanged pair each sit between two textured ones. tests/test_stereo_drive_cpu.py holds the order to that and
    to the differences between neighbouring steps that make a carried-over plane visible."""
    a, b = SPECKLES[1], SPECKLES[2]
    return [("shift 5", "box", None, "internal"),
            ("non-finite", "box", b, "caller"),
            ("occluding step 2/20", "sgm4", b, "internal"),
            ("exchanged", "sgm8", None, "internal"),
            ("occluding step 2/20", "sgm8", None, "caller"),
            ("constant", "sgm8", None, "caller"),
            ("occluding step 4/12", "sgm4", b, "internal"),
            ("non-finite", "box", None, "caller"),
            ("exchanged", "sgm8", None, "internal"),
            ("occluding step 2/20", "sgm4", None, "caller"),
            ("shift 17", "sgm8", b, "internal"),
            ("exchanged", "sgm8", a, "caller"),
            ("shift 17", "sgm8", None, "internal"),
            ("occluding step 4/12", "box", None, "caller"),
            ("shift 17", "sgm4", None, "internal"),
            ("periodic", "box", None, "caller"),
            ("non-finite", "sgm4", None, "internal")]


@functools.lru_cache(maxsize=None)
def _step_model(pair, mode, speckle):
    L, R = sequence_pairs()[pair]
    return filtered(front_model(MODES[mode], L, R, sequence_params()), speckle)


def step_model(index):
    """filtered(front_model) of step `index` alone; shared and read-only."""
    pair, mode, speckle, _ = sequence_steps()[index]
    return _step_model(pair, mode, speckle)
