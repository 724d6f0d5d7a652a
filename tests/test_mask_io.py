"""Region-restricted editing (`--inpainting_mode` with a user mask), the parts that can be checked without a GPU: the mask loader of
scripts/sampling/util.py (directory, .gif, one image; keyframe selection; Pillow's NEAREST byte for byte), the command-line surface of
both entry points, and the four C-ABI entry points of csrc/mask.hip — declared, exported, bound, arguments validated before any HIP
call, and the IEEE divide present in the compiled object."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MASK_SYMBOLS = ("ccedit_mask_resize_nearest", "ccedit_mask_latent", "ccedit_inpaint_blend", "ccedit_mask_composite")


@pytest.fixture(scope="module")
def lib():
    from ccedit_amd.csrc.build import build
    build(force=False, verbose=False)
    from ccedit_amd import hip
    return hip.lib()


def _masks(n=23, h=40, w=56):
    """n grey-level mask frames: a box that moves with the frame index over a noisy background, values on both sides of 128."""
    rs = np.random.RandomState(7)
    out = []
    for i in range(n):
        m = rs.randint(0, 128, (h, w)).astype(np.uint8)                 # background: below the threshold
        box = m[5 + i % 7: 25 + i % 7, 3 + i: 20 + i]
        box[...] = rs.randint(128, 256, box.shape)
        out.append(m)
    return out


def _binary(m):
    return np.where(m >= 128, 255, 0).astype(np.uint8)


def _pil_nearest(m, h, w):
    from PIL import Image
    return np.array(Image.fromarray(m).resize((w, h), Image.NEAREST))


# ---- 1. load_video_mask ---------------------------------------------------------------------
@pytest.mark.parametrize("size", [(40, 56), (24, 40), (64, 96), (37, 53)])
def test_load_video_mask_directory_gif_and_single_image(tmp_path, size):
    from PIL import Image
    from scripts.sampling.util import keyframe_indices, load_video_mask
    ms = _masks()
    d = tmp_path / "m"
    d.mkdir()
    for i, m in enumerate(ms):
        Image.fromarray(m).save(str(d / f"{i:03d}.png"))
    frames = [Image.fromarray(_binary(m)) for m in ms]                      # (a gif keeps a black / white frame exactly)
    frames[0].save(str(tmp_path / "m.gif"), save_all=True, append_images=frames[1:], duration=50, loop=0)
    Image.fromarray(ms[4]).save(str(tmp_path / "one.png"))
    for fps, T in ((20, 3), (20, 5), (3, 23)):          # gap 7 (3 keyframes), gap 7 with too few frames (linspace), every frame
        idx = keyframe_indices(23, fps, 3, T)
        want = np.stack([_pil_nearest(_binary(ms[i]), *size) for i in idx])
        for path in (str(d), str(tmp_path / "m.gif")):
            got = load_video_mask(path, fps, 3, T, size, 23)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (T,) + size
            assert np.array_equal(got.numpy(), want), path
        one = load_video_mask(str(tmp_path / "one.png"), fps, 3, T, size, 23)
        assert tuple(one.shape) == (T,) + size
        assert np.array_equal(one.numpy(), np.stack([_pil_nearest(_binary(ms[4]), *size)] * T))
    assert set(np.unique(load_video_mask(str(d), 20, 3, 3, size, 23).numpy())) <= {0, 255}


def test_load_video_mask_accepts_rgb_and_rejects_a_wrong_frame_count(tmp_path):
    from PIL import Image
    from scripts.sampling.util import load_video_mask
    ms = _masks(9)
    d = tmp_path / "m"
    d.mkdir()
    for i, m in enumerate(ms):
        Image.fromarray(np.stack([m, m, m], -1)).save(str(d / f"{i:03d}.png"))          # an RGB mask: its luminance is taken
    got = load_video_mask(str(d), 9, 3, 3, None, 9)
    assert np.array_equal(got.numpy(), np.stack([_binary(ms[i]) for i in (0, 3, 6)]))
    with pytest.raises(ValueError, match="9 frames.*12"):
        load_video_mask(str(d), 9, 3, 3, None, 12)
    with pytest.raises(ValueError):
        load_video_mask(str(tmp_path / "nothing.txt"), 9, 3, 3, None, 9)


@pytest.mark.parametrize("n_in,n_out", [(40, 40), (40, 24), (56, 96), (6, 9), (9, 6), (270, 128), (1080, 512), (1920, 768), (53, 37), (7, 100),
                                        (3, 2), (512, 768), (1373, 1242), (881, 1999)])
def test_nearest_index_table_is_pillows(n_in, n_out):
    """packing.pil_nearest_index (the table ccedit_mask_resize_nearest gathers with) against Pillow itself on an index ramp."""
    from PIL import Image
    from ccedit_amd.packing import pil_nearest_index
    tab = pil_nearest_index(n_in, n_out)
    assert tab.dtype == np.int32 and tab.shape == (n_out,) and tab.min() >= 0 and tab.max() < n_in
    ramp = np.arange(n_in, dtype=np.int32)[None].repeat(2, 0)
    assert np.array_equal(np.array(Image.fromarray(ramp).resize((n_out, 2), Image.NEAREST))[0], tab)
    num = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in                             # floor((i + 0.5) in / out) in integers = num // den
    den = 2 * n_out
    tie = num % den == 0                                                                # the position is an integer: Pillow's running sum in
    assert np.array_equal(tab[~tie], (num // den)[~tie])                                # double may land just below it, nowhere else
    assert ((tab[tie] == (num // den)[tie]) | (tab[tie] == (num // den)[tie] - 1)).all()


# ---- 2. command line ------------------------------------------------------------------------
def _entry_points():
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return S, R


def test_both_entry_points_accept_the_mask_flags():
    for mod in _entry_points():
        a = mod.parse_args([])
        assert a.mask_path == "" and a.mask_root == "" and a.mask_composite is False and a.inpainting_mode is False
        a = mod.parse_args(["--inpainting_mode", "--mask_path", "m.png", "--mask_root", "masks", "--mask_composite"])
        assert a.inpainting_mode and a.mask_path == "m.png" and a.mask_root == "masks" and a.mask_composite is True
        with pytest.raises(SystemExit) as e:          # argparse's own error exit
            mod.parse_args(["--mask_composite"])
        assert e.value.code == 2
    assert _entry_points()[1].parse_args(["--prior_type", "video_ref"]).prior_type == "video_ref"


def test_inpainting_mode_without_a_mask_still_raises(tmp_path):
    S, _ = _entry_points()
    args = S.parse_args(["--inpainting_mode", "--mask_root", str(tmp_path / "masks")])
    video = str(tmp_path / "clips" / "fox")
    assert S.find_mask(args, video) is None
    with pytest.raises(NotImplementedError) as e:
        S.clip_masks(args, [video], torch.device("cpu"))
    for place in ("--mask_path", "--mask_root", ".mask.png"):
        assert place in str(e.value)
    with pytest.raises(NotImplementedError, match="--mask_path"):          # the sampling function itself, should a caller get that far
        S.sample_one(args, None, None, {}, {}, torch.zeros(1, 4, 3, 8, 8), keyframes=torch.zeros(1, 3, 3, 64, 64))


def test_mask_lookup_mirrors_the_depth_lookup(tmp_path):
    S, _ = _entry_points()
    clips = tmp_path / "clips"
    (clips / "fox").mkdir(parents=True)
    video = str(clips / "fox")
    mk = lambda *a: S.parse_args(["--inpainting_mode", *a])
    assert S.find_mask(mk(), video) is None
    (clips / "fox.mask").mkdir()
    assert S.find_mask(mk(), video) == str(clips / "fox.mask")
    (clips / "fox.mask.png").write_bytes(b"")
    assert S.find_mask(mk(), video) == str(clips / "fox.mask.png")                   # order: .mask.png, .mask.gif, .mask/
    assert S.find_mask(mk(), video + ".gif") == str(clips / "fox.mask.png") == S.find_mask(mk(), video + ".mp4")
    root = tmp_path / "masks"
    (root / "fox").mkdir(parents=True)
    assert S.find_mask(mk("--mask_root", str(root)), video) == str(root / "fox")     # --mask_root before the video's neighbours
    (root / "fox.gif").write_bytes(b"")
    assert S.find_mask(mk("--mask_root", str(root)), video) == str(root / "fox.gif")
    assert S.find_mask(mk("--mask_root", str(root), "--mask_path", "given.png"), video) == "given.png"      # --mask_path first


# ---- 3. C ABI -------------------------------------------------------------------------------
def test_mask_symbols_declared_exported_and_bound(lib):
    from ccedit_amd import hip, ops, packing
    from ccedit_amd.csrc import build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in MASK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/ccedit_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in hip.EXPORTS
    for name in ("mask_resize_nearest", "mask_latent", "inpaint_blend", "mask_composite"):
        assert callable(getattr(ops, name))
    assert callable(packing.pil_nearest_index)
    assert "mask.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["mask.hip"]
    assert not any("fast" in f or "contract=fast" in f for f in build.EXTRA_FLAGS["mask.hip"])
    assert lib.ccedit_abi_version() == 12          # additive: the ABI version does not move


def test_mask_entry_points_validate_before_any_hip_call(lib):
    """Null pointers and impossible sizes: negative code + message, no launch (there is no GPU here)."""
    P = 64          # any non-null, 8-byte aligned "pointer": nothing is dereferenced before the checks fail

    def err():
        return lib.ccedit_last_error()
    assert lib.ccedit_mask_resize_nearest(None, P, P, P, 1, 8, 8, 4, 4, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_resize_nearest(P, P, P, None, 1, 8, 8, 4, 4, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_resize_nearest(P, P, P, P, 0, 8, 8, 4, 4, None) == -1 and b"positive" in err()
    assert lib.ccedit_mask_resize_nearest(P, P, P, P, 1, 8, 8, 4, -4, None) == -1 and b"positive" in err()
    assert lib.ccedit_mask_resize_nearest(P, P, P, P, 1 << 20, 1 << 10, 1 << 10, 4, 4, None) == -1 and b"2^31" in err()
    assert lib.ccedit_mask_latent(None, P, 1, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_latent(P, None, 1, 8, 8, None) == -1
    assert lib.ccedit_mask_latent(P, P, 0, 8, 8, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent(P, P, 1, 12, 8, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent(P, P, 1, 8, 20, None) == -1 and b"multiples of 8" in err()
    assert lib.ccedit_mask_latent(P + 4, P, 1, 8, 8, None) == -1 and b"8-byte aligned" in err()
    assert lib.ccedit_inpaint_blend(None, P, P, P, P, 1, 4, 64, 1.0, 1.5, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_inpaint_blend(P, P, None, P, P, 1, 4, 64, 1.0, 1.5, None) == -1
    assert lib.ccedit_inpaint_blend(P, P, P, None, P, 1, 4, 64, 1.0, 1.5, None) == -1
    assert lib.ccedit_inpaint_blend(P, P, P, P, P, 1, 0, 64, 1.0, 1.5, None) == -1 and b"C=0" in err()
    assert lib.ccedit_inpaint_blend(P, P, P, P, P, 1, 4, 0, 1.0, 1.5, None) == -1 and b"P=0" in err()
    assert lib.ccedit_inpaint_blend(P, P, P, P, P, 1, 4, 64, 1.0, 0.0, None) == -1 and b"must be positive" in err()
    assert lib.ccedit_mask_composite(P, None, P, P, 1, 64, None) == -1 and b"null pointer" in err()
    assert lib.ccedit_mask_composite(P, P, P, P, 0, 64, None) == -1 and b"B=0" in err()
    assert lib.ccedit_mask_composite(P, P, P, P, 1, 0, None) == -1


def test_mask_object_divides_by_the_ieee_sequence(lib):
    """csrc/mask.hip: the known content is (x0 + noise * sigma) / s with one rounding per operation.  What the gfx950 object shows
    (hipcc of ROCm 7): per division two v_div_scale_f32, one v_rcp_f32 refined by v_fma_f32 / v_fmac_f32, v_div_fmas_f32 and
    v_div_fixup_f32 — the correctly rounded sequence; its numerator comes out of a v_add_f32 whose operand is a v_mul_f32 (no fused
    multiply-add in front of the division).  The object holds further v_rcp_f32 / v_fma_f32: the index arithmetic's 64-bit integer
    divisions, which have no v_add_f32 — so "one v_add_f32 per division" is the statement that no product was contracted into a sum."""
    import shutil
    import subprocess
    import tempfile
    from ccedit_amd.csrc import build
    obj = os.path.join(build.HERE, "mask.o")
    if not (os.path.exists(build.OBJDUMP) and os.path.exists(obj)):
        pytest.skip("llvm-objdump or the object file not present")
    with tempfile.TemporaryDirectory() as tmp:
        o = shutil.copy(obj, tmp)
        subprocess.run([build.OBJDUMP, "--offloading", o], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        dis = "".join(subprocess.run([build.OBJDUMP, "-d", os.path.join(tmp, f)], capture_output=True, text=True, check=False).stdout
                      for f in os.listdir(tmp) if "amdgcn" in f)
    ops_ = re.findall(r"^\s+(v_[a-z0-9_]+|global_store\w*)", dis, flags=re.M)
    n = {k: sum(1 for o in ops_ if o.startswith(k)) for k in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_add_f32", "global_store")}
    assert n["global_store"] > 0
    assert n["v_div_fixup_f32"] >= 5, n          # four lanes of the 16-byte variant + the one-element variant
    assert n["v_div_fmas_f32"] == n["v_div_fixup_f32"] and n["v_div_scale_f32"] == 2 * n["v_div_fixup_f32"], n
    assert n["v_add_f32"] == n["v_div_fixup_f32"], n
    # the one-element variant in program order: multiply, add, then the division sequence on the sum
    seq = [o for o in ops_ if o.startswith(("v_mul_f32", "v_add_f32", "v_div_scale_f32", "v_rcp_f32", "v_div_fmas_f32", "v_div_fixup_f32"))]
    pat = ["v_mul_f32", "v_add_f32", "v_div_scale_f32", "v_rcp_f32", "v_div_scale_f32", "v_mul_f32", "v_div_fmas_f32", "v_div_fixup_f32"]
    short = [re.sub(r"_e(32|64)$", "", o) for o in seq]
    assert any(short[i:i + len(pat)] == pat for i in range(len(short))), "no mul -> add -> IEEE division chain in the object"
