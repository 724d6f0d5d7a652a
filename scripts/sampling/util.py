"""Pipeline helpers of the sampling entry points — counterpart of the reference's scripts/sampling/util.py for the
functions on the path (same names, arguments and defaults):

  create_model            util.py:38-42     yaml -> instantiate_from_config(config.model)
  init_sampling           util.py:385-425   (+ get_discretization :428-448, get_guider :451-480, get_sampler :483-556)
  prior_latent            sampling_tv2v.py:371-376, sampling_tv2v_ref.py:415-437   a*encode(keyframes/ref) + b*randn
  sdedit_start            sampling_tv2v.py:436-448   noised latent for --sdedit_denoise_strength
  save_frames / resume log                      sampling_tv2v.py:473-515 (numpy frames instead of mp4: no codec libs offline)

Video decoding, depth annotators, CLIP and the LoRA / base-model merge (util.py:45-272, 689-762) are outside this
build; conditioning arrives as tensors.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import numpy as np
import torch

from ccedit_amd.config import instantiate_from_config, load_config

_DD = "sgm.modules.diffusionmodules."
SAMPLERS_BUILT = ("EulerEDMSampler", "HeunEDMSampler", "EulerAncestralSampler", "DPMPP2SAncestralSampler", "DPMPP2MSampler",
                  "LinearMultistepSampler")


def create_model(config_path: str, device="cuda"):
    config = load_config(config_path)
    with torch.device(device):
        return instantiate_from_config(config.model)


def get_discretization(discretization: str) -> dict:
    if discretization == "LegacyDDPMDiscretization":
        return {"target": _DD + "discretizer.LegacyDDPMDiscretization"}
    if discretization == "EDMDiscretization":
        return {"target": _DD + "discretizer.EDMDiscretization", "params": {"sigma_min": 0.03, "sigma_max": 14.61, "rho": 3.0}}
    raise ValueError(f"unknown discretization {discretization}")


def get_guider(guider_config_target=_DD + "guiders.VanillaCFG", scale=7.5) -> dict:
    return {"target": guider_config_target,
            "params": {"scale": scale, "dyn_thresh_config": {"target": _DD + "sampling_utils.NoDynamicThresholding"}}}


def get_sampler(sampler_name: str, steps: int, discretization_config: dict, guider_config: dict):
    if sampler_name not in SAMPLERS_BUILT:
        raise ValueError(f"unknown sampler {sampler_name}!")
    extra = {"EulerEDMSampler": dict(s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0),       # util.py:484-511
             "HeunEDMSampler": dict(s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0),
             "EulerAncestralSampler": dict(eta=1.0, s_noise=1.0),                              # :512-536
             "DPMPP2SAncestralSampler": dict(eta=1.0, s_noise=1.0),
             "DPMPP2MSampler": dict(),                                                         # :537-543
             "LinearMultistepSampler": dict(order=4)}[sampler_name]                            # :544-553
    return instantiate_from_config(dict(target=_DD + "sampling." + sampler_name, params=dict(
        num_steps=steps, discretization_config=discretization_config, guider_config=guider_config, verbose=True, **extra)))


def init_sampling(sample_steps=50, sampler_name="DPMPP2SAncestralSampler", discretization_name="LegacyDDPMDiscretization",
                  guider_config_target=_DD + "guiders.VanillaCFG", cfg_scale=7.5, img2img_strength=1.0):
    assert 1 <= sample_steps <= 1000, "sample_steps must be between 1 and 1000, but got {}".format(sample_steps)
    sampler = get_sampler(sampler_name, sample_steps, get_discretization(discretization_name),
                          get_guider(guider_config_target=guider_config_target, scale=cfg_scale))
    if img2img_strength < 1.0:
        from scripts.demo.streamlit_helpers import Img2ImgDiscretizationWrapper
        sampler.discretization = Img2ImgDiscretizationWrapper(sampler.discretization, strength=img2img_strength)
    return sampler


def prior_latent(model, randn: torch.Tensor, coeff_x: float, coeff_noise: float, keyframes: Optional[torch.Tensor] = None,
                 ref: Optional[torch.Tensor] = None, prior_type: str = "video") -> torch.Tensor:
    """randn <- coeff_x * prior + coeff_noise * randn, prior = encode_first_stage(keyframes) ['video'], of the
    reference image repeated over T ['ref'], or their sum ['video_ref']."""
    from ccedit_amd import ops
    assert 0.0 < coeff_x <= 1.0, "prior_coefficient_x should be in (0.0, 1.0], but got {}".format(coeff_x)
    t = randn.shape[2]
    if prior_type == "video":
        prior = model.encode_first_stage(keyframes)
    elif prior_type == "ref":
        prior = model.encode_first_stage(ref)[:, :, None].expand(-1, -1, t, -1, -1).contiguous()
    elif prior_type == "video_ref":
        pv = model.encode_first_stage(keyframes)
        pr = model.encode_first_stage(ref)[:, :, None].expand(-1, -1, t, -1, -1).contiguous()
        prior = ops.axpby(pv, pr, 1.0, 1.0)
    else:
        raise NotImplementedError
    return ops.axpby(prior.contiguous(), randn.float().contiguous(), coeff_x, coeff_noise)


def sdedit_start(model, sampler, keyframes: torch.Tensor, noise=None) -> torch.Tensor:
    """z = encode(keyframes); noised_z = (z + randn_like(z) * sigma0) / sqrt(1 + sigma0^2) with sigma0 the first of the
    pruned schedule (hard-coded DDPM-like scaling, as in the reference).  noise: a noise source x -> noise of x's shape to draw from
    in place of torch.randn_like (--noise_warp's carried source); None: as before."""
    from ccedit_amd import ops
    z = model.encode_first_stage(keyframes)
    noise = torch.randn_like(z) if noise is None else noise(z).to(z.dtype)
    sigmas = sampler.discretization(sampler.num_steps)
    s0 = float(sigmas[0])
    inv = 1.0 / float(torch.sqrt(1.0 + sigmas[0].float() ** 2.0))
    return ops.axpby(z.contiguous(), noise.contiguous(), inv, s0 * inv)


def chunk(it, size):
    """util.py:355-357."""
    from itertools import islice
    it = iter(it)
    return iter(lambda: tuple(islice(it, size)), ())


def load_conditioning(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu")


def save_frames(save_path: str, tag: str, x: torch.Tensor) -> str:
    """x: decoded (1,3,T,H,W) in [-1,1] -> <save_path>/result/<tag>.npy with (T,H,W,3) in [0,1] (:473-475)."""
    os.makedirs(os.path.join(save_path, "result"), exist_ok=True)
    x = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
    out = os.path.join(save_path, "result", tag + ".npy")
    np.save(out, x[0].permute(1, 2, 3, 0).cpu().numpy())
    return out


class ResumeLog:
    """log_info.json with the list of finished samples: re-running skips them unless --disable_check_repeat."""

    def __init__(self, save_path: str):
        os.makedirs(save_path, exist_ok=True)
        self.path = os.path.join(save_path, "log_info.json")
        self.log = json.load(open(self.path)) if os.path.exists(self.path) else {"done": []}

    def done(self, tag: str) -> bool:
        return tag in self.log["done"]

    def add(self, tag: str) -> None:
        self.log["done"].append(tag)
        json.dump(self.log, open(self.path, "w"))


# ------------------------------------------------------------------------------------------
# checkpoint ingestion: reference scripts/sampling/util.py:45-272
# ------------------------------------------------------------------------------------------
import re

# kohya "down_blocks_i / attentions_j" and "up_blocks_i / attentions_j" -> sgm input_blocks / output_blocks index
_LORA_IN = {(0, 0): 1, (0, 1): 2, (1, 0): 4, (1, 1): 5, (2, 0): 7, (2, 1): 8}
_LORA_OUT = {(1, 0): 3, (1, 1): 4, (1, 2): 5, (2, 0): 6, (2, 1): 7, (2, 2): 8, (3, 0): 9, (3, 1): 10, (3, 2): 11}
_RE_TE = re.compile(r"^lora_te_text_model_encoder_layers_(\d+)_(self_attn_([qkv]|out)_proj|mlp_(fc1|fc2))$")
_RE_UNET = re.compile(r"^lora_unet_(?:(down|up)_blocks_(\d+)|mid_block)_attentions_(\d+)_(.+)$")
_RE_TAIL = re.compile(r"^(?:proj_(in|out)|transformer_blocks_(\d+)_(?:(attn[12])_to_(?:([qkv])|out_(\d+))|ff_net_(\d+)(?:_(proj))?))$")


def lora_target_key(key: str) -> str:
    """State-dict key of the weight a kohya-format LoRA tensor (`<module>.lora_up/down.weight`) is merged into."""
    mod = key.split(".")[0]
    m = _RE_TE.match(mod)
    if m:
        layer = m.group(1)
        leaf = f"self_attn.{m.group(3)}_proj" if m.group(3) else f"mlp.{m.group(4)}"
        return f"conditioner.embedders.0.transformer.text_model.encoder.layers.{layer}.{leaf}.weight"
    m = _RE_UNET.match(mod)
    t = _RE_TAIL.match(m.group(4)) if m else None
    if not (m and t):
        raise ValueError("Unknown key: ", key)
    if m.group(1) is None:
        base = "model.diffusion_model.middle_block.1"
    else:
        table, name = (_LORA_IN, "input_blocks") if m.group(1) == "down" else (_LORA_OUT, "output_blocks")
        base = f"model.diffusion_model.{name}.{table[(int(m.group(2)), int(m.group(3)))]}.1"
    if t.group(1):
        return f"{base}.proj_{t.group(1)}.weight"
    tb = f"{base}.transformer_blocks.{t.group(2)}"
    if t.group(3):
        return f"{tb}.{t.group(3)}.to_{t.group(4)}.weight" if t.group(4) else f"{tb}.{t.group(3)}.to_out.{t.group(5)}.weight"
    return f"{tb}.ff.net.{t.group(6)}" + (".proj" if t.group(7) else "") + ".weight"


def convert_load_lora(sd_state_dict: Dict[str, torch.Tensor], state_dict: Dict[str, torch.Tensor],
                      LORA_PREFIX_UNET="lora_unet", LORA_PREFIX_TEXT_ENCODER="lora_te", alpha=0.6):
    """util.py:115-272: W += alpha * (lora_up @ lora_down) for every LoRA pair, in place in `sd_state_dict`
    (1x1-conv projections keep their (O, I, 1, 1) shape; `.alpha` entries are ignored like the reference does)."""
    if (LORA_PREFIX_UNET, LORA_PREFIX_TEXT_ENCODER) != ("lora_unet", "lora_te"):
        raise NotImplementedError("non-default LoRA prefixes")
    done = set()
    for key in state_dict:
        if ".alpha" in key or key in done:
            continue
        up_key = key.replace("lora_down", "lora_up")
        down_key = key.replace("lora_up", "lora_down")
        up, down = state_dict[up_key].to(torch.float32), state_dict[down_key].to(torch.float32)
        target = lora_target_key(key)
        if up.dim() == 4:
            delta = torch.mm(up.squeeze(3).squeeze(2), down.squeeze(3).squeeze(2)).unsqueeze(2).unsqueeze(3)
        else:
            delta = torch.mm(up, down)
        sd_state_dict[target] += alpha * delta
        done.update((up_key, down_key))
    return sd_state_dict


def read_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(("ckpt", ".pt", ".pth")):
        sd = torch.load(path, map_location="cpu")
        if "deepspeed" in path:
            return {k.replace("_forward_module.", ""): v for k, v in sd.items()}
        return sd["state_dict"] if "state_dict" in sd else sd
    if path.endswith("safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    raise NotImplementedError(f"Unknown checkpoint format: {path}")


def remap_checkpoint_keys(sd: Dict[str, torch.Tensor], newbasemodel: bool = False) -> Dict[str, torch.Tensor]:
    """util.py:63-82: VAE copies nested under conditioner embedders lose that prefix; with `newbasemodel` (a plain
    SD-1.5 checkpoint as base) `cond_stage_model.*` becomes `conditioner.embedders.0.*`."""
    out = {}
    for k, v in sd.items():
        if k.startswith("conditioner.embedders.") and "first_stage_model" in k:
            k = k[k.find("first_stage_model"):]
        if newbasemodel and "cond_stage_model" in k:
            k = k.replace("cond_stage_model", "conditioner.embedders.0")
        out[k] = v
    return out


def model_load_ckpt(model, path: str, newbasemodel: bool = False):
    """util.py:45-112: non-strict load with the key surgery above; LoRA tensors embedded in the checkpoint
    (`lora*` keys, e.g. majicmixRealistic) are merged at alpha = 0.8 like the reference does, then loaded."""
    sd = remap_checkpoint_keys(read_checkpoint(path), newbasemodel)
    lora = {k: v for k, v in sd.items() if k.startswith("lora")}
    if lora:
        for k in lora:
            del sd[k]
        convert_load_lora(sd_state_dict=sd, state_dict=lora, alpha=0.8)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if newbasemodel:
        unwanted = ["temporal", "controlnet", "conditioner.embedders.1."]
        missing = [k for k in missing if all(s not in k for s in unwanted)]
    print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")
    if missing:
        print(f"Missing Keys: {missing}")
    if unexpected:
        print(f"Unexpected Keys: {unexpected}")
    return model


def load_lora_file(model, lora_path: str, strength: float) -> None:
    """sampling_tv2v.py:212-236: merge a kohya .safetensors LoRA into the model's weights at `strength`."""
    if not lora_path.endswith(".safetensors"):
        raise NotImplementedError
    from safetensors.torch import load_file
    lora_sd = load_file(lora_path)
    if not all("lora" in k for k in lora_sd):
        raise ValueError(f"The model you provided in [{lora_path}] is not a LoRA model. ")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(convert_load_lora(sd, lora_sd, alpha=strength))


def load_vae_file(model, vae_path: str) -> None:
    """sampling_tv2v.py:238-260: replacement first stage (.pt with `state_dict`, or .safetensors)."""
    if vae_path.endswith(".pt"):
        vae_sd = torch.load(vae_path, map_location="cpu")["state_dict"]
    elif vae_path.endswith(".safetensors"):
        from safetensors.torch import load_file
        vae_sd = load_file(vae_path)
    else:
        raise ValueError("Cannot load vae model from {}".format(vae_path))
    print("msg of loading vae: ", model.first_stage_model.load_state_dict(vae_sd, strict=False))


# ------------------------------------------------------------------------------------------
# frame / video I/O: reference scripts/sampling/util.py:288-382, 689-762
# Which way a source or a file goes is data: ccedit_amd/video_io.py holds the table of source kinds (directory of frame files, .gif,
# Motion-JPEG .avi, animated .png) with their device decoders, and the table of writers.  The functions here keep the reference's names,
# arguments and arithmetic, and ask there.
# ------------------------------------------------------------------------------------------
from ccedit_amd import video_io                                                    # noqa: E402
from ccedit_amd.video_io import GIF_ENCODERS, HWC3                                 # noqa: E402, F401  (util.py:559-576 is HWC3)


def _decode_rgb_u8(path: str) -> np.ndarray:
    """Image file -> uint8 (H, W, 3) on the host (the decode is Pillow's on both routes)."""
    from PIL import Image
    a = np.array(Image.open(path))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{path}: the device route takes 8-bit RGB images, got {a.dtype} {a.shape}")
    return a


def _upload(frames, device):
    """uint8 frames (list of (h, w, 3) arrays) -> uint8 tensors on `device`: ONE upload of the whole clip when the frames share a size,
    else one (1, h, w, 3) tensor per frame."""
    groups = [np.stack(frames, axis=0)] if len({f.shape for f in frames}) == 1 else [f[None] for f in frames]
    return [torch.from_numpy(np.ascontiguousarray(g)).to(device) for g in groups]


def _files_u8(paths, device, what: str):
    """Image files -> uint8 (n, h, w, 3) tensors on `device`: decoded there where a decoder takes the whole clip, else Pillow's frames."""
    on_device = video_io.files_u8_device(video_io.FILES.device, paths, device, what)
    return on_device if on_device is not None else _upload([_decode_rgb_u8(p) for p in paths], device)


def _clip_u8(kind, video_path: str, device, select=None, gif_decoder: str = "pillow"):
    """A video in one file (all frames, or those at select(number of frames)) -> [uint8 (N, h, w, 3) on `device`]: decoded there where a
    decoder takes the whole clip, else Pillow's frames, selected before the upload.  gif_decoder="device": the kind's opt-in decoders
    (a .gif: ccedit_amd/gifdec.py) are asked too."""
    on_device = video_io.clip_u8_device(video_io.decoders_of(kind, gif_decoder), video_path, device, select)
    if on_device is not None:
        return [on_device]
    frames = kind.u8(video_path)
    return _upload(list(frames if select is None else frames[select(frames.shape[0])]), device)


def _u8_to_float(groups, size) -> torch.Tensor:
    """uint8 (n, h, w, 3) tensors on the device -> fp32 (T, 3, H, W) in [-1, 1]: one launch per resize pass for the whole clip when the
    frames share a size (else per frame), Pillow's 8-bit bicubic + x / 255 * 2 - 1 in ccedit_amd/csrc/pixel.hip — bit-identical to
    load_img on the host."""
    from ccedit_amd import ops
    if len(groups) > 1:
        assert size, "frames of different sizes need a target size"
    out = [ops.resize_u8_pil(g.contiguous(), size or tuple(g.shape[1:3]), to_float=True) for g in groups]
    return (out[0] if len(out) == 1 else torch.cat(out, dim=1)).permute(1, 0, 2, 3)


def load_img(p_cond_img: str, size: tuple = None, device=None) -> torch.Tensor:
    """util.py:360-382: image file -> (1, 3, H, W) in [-1, 1], optional bicubic resize to size = (H, W).
    device=None: Pillow and torch on the host, as the reference.  With a device a .jpg / .jpeg / .png file is decoded there
    (ccedit_amd/jpegdec.py, pngdec.py), any other image is decoded by Pillow and uploaded as uint8; either is resized / scaled there
    (same values, bit for bit)."""
    if device is not None:
        if size:
            assert len(size) == 2, "size should be (H, W)"
        return _u8_to_float(_files_u8([p_cond_img], device, p_cond_img), size)
    from PIL import Image
    img = Image.open(p_cond_img)
    if size:
        assert len(size) == 2, "size should be (H, W)"
        h, w = size
        img = img.resize((w, h), Image.BICUBIC)
    t = torch.from_numpy(np.array(img)).permute(2, 0, 1).unsqueeze(0).float() / 255.0
    return torch.clamp(t * 2.0 - 1.0, -1.0, 1.0)


def keyframe_indices(num_allframes: int, original_fps: int, target_fps: int, num_keyframes: int) -> np.ndarray:
    """util.py:708-720 / 735-745: every round(original_fps / target_fps)-th frame, the first `num_keyframes` of them;
    when the video is too short, `num_keyframes` indices spread evenly over it instead."""
    gap = int(np.round(original_fps / target_fps).astype(int))
    assert gap > 0, f"gap {gap} should be positive."
    idx = list(range(0, num_allframes, gap))
    if len(idx) < num_keyframes:
        print("[WARNING]: not enough keyframes, use linspace instead. "
              f"len(keyindexs): [{len(idx)}] < num_keyframes [{num_keyframes}]")
        return np.linspace(0, num_allframes - 1, num_keyframes).astype(int)
    return np.asarray(idx[:num_keyframes])


def load_video_frames_u8(video_path: str, size: tuple, device, gif_decoder: str = "pillow") -> torch.Tensor:
    """(not in the reference) ALL frames of what load_video_keyframes reads -> uint8 (F, H, W, 3) on `device` at size = (H, W): the
    source side of --propagate.  JPEG and PNG sources (a directory of such files, the frames of an .avi or of an animated .png) are
    decoded on the device (ccedit_amd/jpegdec.py, pngdec.py: only the compressed bytes go up; Pillow's bytes exactly); everything else,
    and a clip the device decoder declines, is decoded by Pillow on the host and uploaded.  The frames reach the output size by the
    routes of the keyframes — image files by Pillow's 8-bit bicubic (ops.resize_u8_pil), the frames of a video in one file by the fp32
    bicubic of F.interpolate and then the nearest byte (ops.resize_bicubic, ops.frames_to_u8 with rounding).
    gif_decoder="device": a .gif is decoded on the device too (ccedit_amd/gifdec.py: Pillow's bytes exactly; a file outside its subset
    goes through Pillow with one line on stderr); "pillow" (the default): a .gif is Pillow's, as before."""
    from ccedit_amd import ops
    assert device is not None and size and len(size) == 2, "load_video_frames_u8 works on a device, size should be (H, W)"
    kind = video_io.kind_of(video_path)
    if kind is video_io.FILES:
        groups = _files_u8([os.path.join(video_path, f) for f in sorted(os.listdir(video_path))], device, video_path)
        out = [ops.resize_u8_pil(g.contiguous(), size) for g in groups]
        return out[0] if len(out) == 1 else torch.cat(out, dim=0)
    x = ops.resize_bicubic(_u8_to_float(_clip_u8(kind, video_path, device, gif_decoder=gif_decoder), None).contiguous(), size)      # (F, 3, h, w) in [-1, 1] -> (F, 3, H, W)
    return ops.frames_to_u8(x.permute(1, 0, 2, 3)[None].contiguous(), rounding=True)[0]


def load_video_keyframes(video_path: str, original_fps: int, target_fps: int, num_keyframes: int, size: tuple = None,
                         device=None, gif_decoder: str = "pillow") -> torch.Tensor:
    """util.py:689-762: directory of frame images, a .gif, a Motion-JPEG .avi or an animated .png -> keyframes (T, 3, H, W) in [-1, 1].
    device=None: everything on the host, as the reference.  With a device, JPEG and PNG sources (such files, the frames of an .avi or
    of an animated .png) are decoded there (ccedit_amd/jpegdec.py, pngdec.py: only the compressed bytes go up, the frames are Pillow's
    byte for byte); everything else, and a clip the device decoder declines, is decoded by Pillow on the host and uploaded once as
    uint8.  Either way the keyframes are resized / scaled by the kernels of ccedit_amd/csrc/pixel.hip: image files exactly as on the
    host (Pillow's 8-bit bicubic), the frames of a video in one file by the fp32 bicubic of F.interpolate (equal to fp32 rounding).
    gif_decoder="device" (with a device; not in the reference): a .gif is decoded on the device as well (ccedit_amd/gifdec.py: the same
    bytes as Pillow's); "pillow" (the default) is the route as before."""
    if device is not None and size:
        assert len(size) == 2, "size should be (H, W)"
    select = lambda n: keyframe_indices(n, original_fps, target_fps, num_keyframes)      # noqa: E731
    kind = video_io.kind_of(video_path)
    if kind is video_io.FILES:
        files = sorted(os.listdir(video_path))
        paths = [os.path.join(video_path, files[i]) for i in select(len(files))]
        if device is not None:
            return _u8_to_float(_files_u8(paths, device, video_path), size)
        return torch.cat([load_img(p, size) for p in paths], dim=0)
    if device is not None:
        from ccedit_amd import ops
        x = _u8_to_float(_clip_u8(kind, video_path, device, select, gif_decoder), None).contiguous()       # uint8 -> x / 255 * 2 - 1, (T, 3, h, w)
        return ops.resize_bicubic(x, size) if size else x
    frames = torch.from_numpy(kind.u8(video_path)).permute(0, 3, 1, 2).float() / 255.0
    frames = frames[select(frames.shape[0])]
    frames = torch.clamp(frames * 2.0 - 1.0, -1.0, 1.0)
    if size:
        assert len(size) == 2, "size should be (H, W)"
        frames = torch.nn.functional.interpolate(frames, size=size, mode="bicubic", align_corners=False)
    return frames


def count_video_frames(video_path: str) -> int:
    """Number of frames of what load_video_keyframes reads: files of a directory, frames of a .gif, a Motion-JPEG .avi or an animated .png."""
    return video_io.kind_of(video_path, mp4_hint=False).count(video_path)


_MASK_IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")


def load_video_mask(mask_path: str, original_fps: int, target_fps: int, num_keyframes: int, size: tuple = None, num_allframes: int = None,
                    device=None, all_frames: bool = False, graded: bool = False) -> torch.Tensor:
    """The edit mask of a clip -> uint8 (T, H, W) holding 0 (keep the original) or 255 (edit): the reference's
    x = x * mask + img_orig * (1 - mask) with white = 1.  (The reference leaves the mask to the user: sampling_tv2v.py:385-407.)
    mask_path: what load_video_keyframes accepts — a directory of images, a .gif or a Motion-JPEG .avi, one mask per frame of the VIDEO: `num_allframes`
    (None: not checked) must equal its frame count, the keyframes are selected by the same `keyframe_indices` rule as the frames — or
    ONE image file, used for every keyframe.  Any image mode is taken through its luminance (`convert("L")`); a value >= 128 is white.
    Every kind is decoded by Pillow on the host (an .avi through ccedit_amd.mjpeg.decode_avi_u8).
    Resize to size = (H, W) is nearest-neighbour on the binarised mask, src = floor((dst + 0.5) * in / out) (Pillow's NEAREST, its
    running sum in double included: ccedit_amd/packing.py pil_nearest_index).  device=None: Pillow on the host.  With a device the
    binarised keyframe masks are uploaded once and gathered there (ccedit_mask_resize_nearest): identical bytes.
    all_frames (--propagate): the masks of ALL frames of the video, (num_allframes, H, W), instead of the keyframes'; one image file is
    repeated num_allframes times (which must then be given).
    graded (--mask_graded): the luminance bytes as they are, no cut at 128 — byte g is the edit strength g / 255; the nearest resize
    keeps bytes on both routes."""
    from PIL import Image
    if size:
        assert len(size) == 2, "size should be (H, W)"

    def lum(img):
        a = np.array(img.convert("L"))
        return np.ascontiguousarray(a, dtype=np.uint8) if graded else np.where(a >= 128, 255, 0).astype(np.uint8)

    kind = video_io.kind_of(mask_path, missing_ok=True)
    if kind is not None:
        n, pick = kind.pil(mask_path, lum)
    elif mask_path.lower().endswith(_MASK_IMAGE_EXT):
        one = lum(Image.open(mask_path))
        n, pick = None, lambda i: one
    else:
        raise ValueError(f"Unsupported mask format: {mask_path}. Only support directory, .gif, .avi (Motion-JPEG) and one image file {_MASK_IMAGE_EXT}.")
    if all_frames and n is None and num_allframes is None:
        raise ValueError("load_video_mask(all_frames=True) of one image needs num_allframes")
    if n is not None and num_allframes is not None and n != num_allframes:
        raise ValueError(f"mask {mask_path} has {n} frames, the video has {num_allframes}: a mask sequence needs one mask per frame "
                         "(or give one image for all frames)")
    if n is None:
        masks = [pick(0)] * (num_allframes if all_frames else num_keyframes)
    else:
        masks = [pick(int(i)) for i in (range(n) if all_frames else keyframe_indices(n, original_fps, target_fps, num_keyframes))]
    if len({m.shape for m in masks}) != 1:
        raise ValueError(f"mask {mask_path}: frames of different sizes {sorted({m.shape for m in masks})}")
    if device is not None:
        from ccedit_amd import ops
        m = torch.from_numpy(np.ascontiguousarray(np.stack(masks, axis=0))).to(device)
        return ops.mask_resize_nearest(m, size) if size and tuple(size) != tuple(m.shape[1:]) else m
    if size and tuple(size) != masks[0].shape:
        h, w = size
        masks = [np.array(Image.fromarray(m).resize((w, h), Image.NEAREST)) for m in masks]
    return torch.from_numpy(np.ascontiguousarray(np.stack(masks, axis=0)))


def save_gif_u8(save_path: str, frames, fps: int, gif_encoder: str = "pillow") -> str:
    """uint8 frames (T, H, W, 3) -> <save_path>/gif/animation-XXXX.gif, numbered and written like perform_save_locally_video's.
    gif_encoder='device' (not in the reference): the frames, a device tensor or a host array that is uploaded once, are quantised and
    LZW-coded on the device; 'pillow' (the default) writes the file with Pillow, byte for byte as before."""
    return video_io.save_u8(save_path, video_io.writer_of("gif", gif_encoder), frames, fps)


def save_avi_u8(save_path: str, frames, fps: int, quality: int = 90) -> str:
    """uint8 frames (T, H, W, 3), on the device or on the host (then uploaded) -> <save_path>/mjpeg/animation-XXXX.avi, numbered like
    save_gif_u8's files: Motion-JPEG, every frame encoded on the device (ccedit_amd/mjpeg.py), only the compressed bytes come back."""
    return video_io.save_u8(save_path, video_io.writer_of("mjpeg"), frames, fps, video_quality=quality)


def save_png_u8(save_path: str, frames, fps: int) -> str:
    """uint8 frames (T, H, W, 3), on the device or on the host (then uploaded) -> <save_path>/png/animation-XXXX.png, numbered like
    save_gif_u8's files: an animated PNG (one frame: a plain PNG) holding exactly these bytes, rows filtered and deflate-coded on the device
    (ccedit_amd/png.py, csrc/png.hip); only the compressed streams come back, the container is written on the host."""
    return video_io.save_u8(save_path, video_io.writer_of("png"), frames, fps)


def perform_save_locally_video(save_path: str, samples: torch.Tensor, fps: int, savetype: str = "gif",
                               return_savepaths: bool = False, save_grid: bool = True, gpu_io: bool = False, signed: bool = False,
                               video_quality: int = 90, gif_encoder: str = "pillow"):
    """util.py:288-352: samples (B, 3, T, H, W) in [0, 1] -> <save_path>/gif/animation-XXXX.gif (+ grid/grid-XXXX.png:
    the T frames side by side).  savetype='mp4' needs a codec library and raises.
    savetype='mjpeg' (not in the reference): <save_path>/mjpeg/animation-XXXX.avi, Motion-JPEG at `video_quality` (1 ... 100), numbered and
    returned like the gifs; the uint8 frames are the gif branch's — made on the host and uploaded, or on the device with gpu_io: the same
    bytes either way — and every frame is encoded on the device (ccedit_amd/mjpeg.py, csrc/mjpeg.hip).
    savetype='png' (not in the reference): <save_path>/png/animation-XXXX.png, a lossless animated PNG of the same uint8 frames, numbered and
    returned like the gifs, coded on the device (ccedit_amd/png.py, csrc/png.hip); any H and W; `video_quality` is ignored.
    gpu_io (savetype='gif', 'mjpeg' or 'png', device tensor): the uint8 frames are made on the device (ccedit_frames_to_u8) and 3 bytes per pixel
    instead of 12 come to the host; the files are byte-identical.  `signed` (with gpu_io only): samples are the decoder's output in
    [-1, 1] and clamp((x + 1) / 2, 0, 1) is part of the same kernel.
    gif_encoder='device' (savetype='gif' only, not in the reference): the gif is quantised and LZW-coded on the device (ccedit_amd/gif.py,
    csrc/gif.hip) from the uint8 frames the Pillow branch would have quantised — with gpu_io they never leave the device, otherwise they
    are uploaded once: the same bytes either way.  File names, numbering, returned paths and the grid PNG are those of 'pillow'."""
    from PIL import Image
    assert samples.dim() == 5, "Expected samples to have shape (B, C, T, H, W)"
    assert savetype in ["gif", "mp4", "npy", "mjpeg", "png"]
    writer = video_io.writer_of(savetype, gif_encoder)             # (the gif_encoder checks; None: npy, mp4)
    assert gpu_io or not signed, "signed samples are only taken on the gpu_io route"
    if savetype == "mp4":
        raise NotImplementedError("mp4 encoding needs imageio-ffmpeg / cv2, not installed here: use savetype='gif'")
    u8 = u8_grid = None
    if gpu_io:
        from ccedit_amd import ops
        if writer is None or not samples.is_cuda:
            raise ValueError("gpu_io saves uint8 frames (savetype='gif') of a device tensor")
        x = samples.detach().float().contiguous()
        u8 = ops.frames_to_u8(x, rounding=False, unit_range=not signed)                                # (B, T, H, W, 3)
        u8 = u8 if writer.on_device else u8.cpu().numpy()                  # (a device writer: the frames stay on the device)
        u8_grid = ops.frames_to_u8(x, rounding=True, unit_range=not signed).cpu().numpy() if save_grid else None
    savepaths = []
    if savetype == "npy":          # (not in the reference) the frames themselves: <save_path>/npy/frames-XXXX.npy, (T, H, W, C) float32 in [0, 1]
        for sample in samples:
            savepaths.append(video_io.next_path(os.path.join(save_path, "npy"), "frames", ".npy"))
            np.save(savepaths[-1], sample.detach().float().cpu().permute(1, 2, 3, 0).numpy())
        return savepaths if return_savepaths else None
    options = {k: v for k, v in dict(video_quality=video_quality, gif_encoder=gif_encoder).items() if k in writer.options}
    for b, sample in enumerate(samples):
        if u8 is None:
            frames_f = sample.detach().float().cpu().permute(1, 2, 3, 0).numpy()          # (T, H, W, C)
        if save_grid:
            # torchvision.utils.save_image(normalize=False, padding=0): x * 255 + 0.5, clamp, uint8
            grid = np.concatenate(list(np.clip(frames_f * 255.0 + 0.5, 0, 255).astype(np.uint8) if u8 is None else u8_grid[b]), axis=1)
            Image.fromarray(grid).save(video_io.next_path(os.path.join(save_path, "grid"), "grid", ".png"))
        savepaths.append(video_io.save_u8(save_path, writer, (255.0 * frames_f).astype(np.uint8) if u8 is None else u8[b], fps, **options))
    return savepaths if return_savepaths else None

