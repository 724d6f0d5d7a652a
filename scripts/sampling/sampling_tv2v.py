#!/usr/bin/env python3
"""TV2V sampling entry point on the MI355X path — counterpart of the reference's
scripts/sampling/sampling_tv2v.py (same flag names for the options on the path; core loop = its lines 333-470,
including the `--prior_coefficient_x` noise prior and the `--sdedit_denoise_strength` branch).

Conditioning producers (CLIP text encoder, MiDaS depth, video decoding) are outside this build (weights / codecs
unavailable offline): pass precomputed tensors with --cond_path — a .pt/.safetensors holding
`tokens`, `tokens_uc` (1,77) int64 CLIP token ids (or precomputed `crossattn`, `crossattn_uc` (1,77,768)), `control_hint` (1,3,T,H,W) in [-1,1] and, for the prior / SDEdit options,
`keyframes` (1,3,T,H,W) in [-1,1] — or use --synthetic for seeded random tensors of the right shapes.  They enter
through `model.conditioner.get_unconditional_conditioning` exactly like the reference's batch dicts.
Outputs: `<save_path>/result/sample_XXXX.npy` (frames in [0,1], (T,H,W,3)) + `log_info.json` resume-skip list.

Job mode (round 6) — the reference script's own surface (sampling_tv2v.py:45-72, 106-204, 264-515): `--prompt` + `--video_path`,
`--prompt_listpath` + `--video_listpath`, `--videos_directory` (sub-directory name = prompt) or the BalanceCC layout `--json_path` +
`--videos_root` (item["Video Type"] / item["Video Name"] + ".mp4", one job per item["Editing"][i]["Target Prompt"], saved under
<save_path>/<Video Type>/<Video Name>/<Target Prompt>); `--num_samples` repeats, `--batch_size` chunks (one CFG-doubled batch of
2 x bs clips per chunk), `--basemodel_listpath` / `--use_default` loop over base models, results in
<save_path>/<basemodel>/{original,result,control_hint}/ + log_info.json (video_paths, keyframes_paths; processed videos are skipped
unless --disable_check_repeat).  What the reference computes with networks that are not part of this build enters as data: the depth
of a clip from `<video>.depth.pt` / `--depth_root/<name>.pt` (raw depth (N,h,w) of ALL frames; normalised by the conditioner's
MiDaS / Zoe recipe), prompts through `--tokenizer_path`; `--synthetic` substitutes the frames' luminance and prompt-seeded token ids.
`--inpainting_mode` (a stub in the reference: "mask should be provided by the user", :385-407) works here with a user's mask —
`--mask_path`, `--mask_root/<video name>.{png,gif}` | `<video name>/`, or `<video stem>.mask.png | .mask.gif | .mask/`; white = edit, black = keep —
through the samplers' sample_inpainting and the kernels of ccedit_amd/csrc/mask.hip; `--mask_composite` puts the original pixels back
outside the mask after decoding; the mask as applied is saved under <save_path>/<basemodel>/mask/.
`--mask_track` (with ONE mask image, painted on source frame `--mask_frame`) gives every source frame its own mask, tracked along the
source's motion on the device (ccedit_amd/masktrack.py, csrc/masktrack.hip); `--mask_dilate R` and `--mask_invert` apply afterwards,
to untracked masks too.
`--mask_auto --source_prompt TEXT` (job mode, with --inpainting_mode) needs no painted mask: the encoded clip is noised and evaluated with
(source prompt, --prompt) in the two halves of one CFG-doubled batch, --mask_auto_samples times, and the mask is where the two predictions
disagree — summed differences scaled by a quantile, thresholded, cleaned by a 3 x 3 x 3 vote over space and time (ccedit_amd/automask.py,
csrc/automask.hip); it then goes where a painted mask goes (--mask_dilate, --mask_invert, --mask_composite, mask/).  --mask_auto_save DIR
writes it as DIR/<video name>/%05d.png per source frame, which --mask_root DIR reads back; log_info.json gains `mask_auto`.  The quality
of such masks on real footage has not been measured.
`--mask_graded` reads the mask's grey levels as edit strengths g / 255 and `--mask_feather R` (0 ... 64 pixels, after --mask_dilate and
--mask_invert) turns whatever mask the run has into such a map by a (2R + 1)^2 mean: a latent cell of strength s is held to the noised
source for the first (1 - s) of the walked schedule and left alone afterwards, and --mask_composite mixes result and original in
proportion to the pixel strengths (ccedit_amd/softmask.py, csrc/softmask.hip); mask/ then holds grey images and log_info.json gains
`mask_graded` and `mask_feather`.  Refused: --mask_graded with --mask_track, a graded run with --propagate --mask_composite or with
WORLD_SIZE > 1.  Image quality is not claimed.
`--noise_warp` carries every noise draw of the run — the start latent, the ancestral / churn noise of every step, the re-injection noise
of --inpainting_mode, the SDEdit start — from keyframe to keyframe along the SOURCE's motion: once per clip an index map says which sample
every latent cell of every keyframe inherits (the matcher of --propagate, every frame reads distinct samples: its noise stays white), and
every draw is gathered through it (ccedit_amd/noisewarp.py, csrc/noisewarp.hip); `--noise_warp_rho R` (0 ... 1, default 1) mixes
sqrt(1 - R^2) of a fresh draw in; log_info.json gains `noise_warp`.  Needs a video and --H, --W multiples of 64; refused with a
reference image and with WORLD_SIZE > 1.  Image quality is not claimed.
`--report_quality` (job mode) measures every clip after it is saved, on the GPU and on the uint8 frames original/ and result/ hold
(ccedit_amd/quality.py, csrc/quality.hip): fidelity of the result to the source keyframes — squared error per channel, PSNR, SSIM on
8 x 8 luma windows; with --inpainting_mode over the pixels the clip's mask keeps — and temporal consistency: the warp error of the result
along the SOURCE's motion between neighbouring keyframes beside the source's own, over the pixels the previous frame shows, with the share
of pixels the motion estimate could follow (keyframes lie original_fps / target_fps source frames apart: that share says how far the
matcher reached).  With --propagate the same over every source frame against result_full/ (`full_rate`).  The report is written to
<save_path>/<basemodel>/quality/<clip number>.json and log_info.json gains `quality`; sizes off the 64 grid and single frames get
`"temporal": null` with the reason.  Refused with WORLD_SIZE > 1.  These are measures of fidelity and steadiness, not of how well the
prompt was followed; on synthetic weights they measure the pipeline, not a model.
`--window_frames T` (with `--window_overlap O`, default T // 2) lifts the limit of one window of keyframes: with `--num_keyframes N` > T the
clip is covered by overlapping windows of T frames, each evaluated by the unchanged network at every sampler evaluation and fused into
one denoised latent of N frames (ccedit_amd/windows.py, csrc/window.hip); everything else — inpainting, SDEdit, the prior mix,
--noise_seed, --gpu_io — runs on the long latent as on a short one, first-stage encode / decode in groups of at most T frames.
`--tile_h TH --tile_w TW` (pixels, multiples of 64; with `--tile_overlap O`, default a quarter of the tile per axis) lifts the limit of one
frame size: with `--H` above TH or `--W` above TW the frame — any multiple of 8 pixels, 720 x 1280 and 1080 x 1920 included — is covered
by overlapping tiles of TH x TW, each evaluated by the unchanged network at every sampler evaluation and fused into one denoised
latent of the frame (ccedit_amd/tiles.py, csrc/tile.hip); everything else — inpainting, SDEdit, the prior mix, --window_frames (inside
every tile), --noise_seed, --gpu_io, masks, the writers — runs on the large latent as on a small one, first-stage encode / decode on whole
frames in groups sized so that no tensor outgrows a plain clip's at tile size.  Exact arithmetic and known shapes are what is claimed;
image quality against a direct evaluation at the large size has not been measured.
`--region_prompt TEXT --region_mask PATH` (a pair per region, up to 7) gives masked regions of the frame prompts of their own — "the bear
becomes a panda, the background becomes a snow field" in ONE run: at every sampler evaluation the unchanged network is evaluated once
per prompt (`--prompt` stays the base prompt and covers whatever the regions leave) and the K + 1 denoised latents are fused into one by a
fixed per-cell blend, feathered over `--region_feather` latent cells (ccedit_amd/regions.py, csrc/region.hip), so there is one latent
and no seam at any step; a region mask is what --mask_path accepts, or with `--region_track` ONE image painted on source frame
`--region_frame` and followed through the clip; everything else — inpainting, SDEdit, the prior mix, --window_frames, --tile_h / --tile_w,
the writers — runs as before.  One clip per invocation; K + 1 network evaluations per sampler evaluation; image quality is not claimed.
`--prompt_chunks N` (1 ... 4) lets every prompt of the run — positive, negative, region prompts, the job lists' — use up to N chunks of
77 tokens instead of being truncated at 75 tokens: chunks end after a nearby comma or at the word BREAK, every chunk is encoded on its
own and the network sees a context of 77 n rows, one n for all prompts of a clip (ccedit_amd/prompt.py); a prompt that needs more is
refused.  `--prompt_syntax weighted` reads `(x)`, `[x]`, `(x:1.3)` as emphasis, applied to the text encoder's output (csrc/prompt.hip).
Conditioning files may hold `tokens` / `tokens_uc` of (1, 77 n) and `token_weights` / `token_weights_uc`; log_info.json gains `prompts`.
With the defaults (1, plain) the text path is the one it was; a prompt it truncates is announced by one `[prompt]` line on stderr.
Launched under torch.distributed (RANK / WORLD_SIZE), the chunks are dealt round-robin to the ranks (BASELINE.json config 5:
independent clips, one per GPU, no collective — ccedit_amd.parallel.shard_clips).
`--propagate` (job mode, --save_type gif, mjpeg or png) adds the frames BETWEEN the keyframes: every source frame from the first to the last keyframe
gets an edited frame, the two neighbouring edited keyframes carried along motion estimated on the source (ccedit_amd/propagate.py,
csrc/propagate.hip), written to <save_path>/<basemodel>/result_full/gif/ (or mjpeg/, png/) at --original_fps; log_info.json gains `fullrate_paths`.
`--save_type mjpeg` writes true-colour video: Motion-JPEG in an .avi, every frame encoded on the GPU (ccedit_amd/mjpeg.py, csrc/mjpeg.hip) at
--video_quality; such an .avi is also a video SOURCE wherever a .gif is.
`--save_type png` writes lossless true-colour video: one animated PNG per clip, filtered and deflate-coded on the GPU (ccedit_amd/png.py,
csrc/png.hip); any H and W; an animated .png is also a video SOURCE wherever a .gif is.
`--gif_encoder device` (with --save_type gif) quantises and LZW-codes every .gif a job writes on the GPU (ccedit_amd/gif.py, csrc/gif.hip);
the default, `pillow`, writes them on the host as before.
`--gif_decoder device` (with --gpu_io) decodes every .gif SOURCE on the GPU (ccedit_amd/gifdec.py, csrc/gifdec.hip: a table of LZW codes, one
lane per code, frames composited on the device; the same bytes as Pillow's); a file outside its subset, and the default `pillow`, go
through Pillow on the host as before.  Masks stay Pillow's.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GUIDER = "sgm.modules.diffusionmodules.guiders.VanillaCFGTV2V"


class _StoreGiven(argparse.Action):
    """store, and note on the namespace (<dest>_given) that the flag was on the command line: a default cannot tell."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def add_common_args(p: argparse.ArgumentParser) -> None:
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--config_path", type=str, default="")
    p.add_argument("--ckpt_path", type=str, default="")
    p.add_argument("--use_default", action="store_true", help="use default ckpt at first")
    p.add_argument("--basemodel_path", type=str, default="", help="load a new base model instead of original sd-1.5")
    p.add_argument("--basemodel_listpath", type=str, default="")
    p.add_argument("--lora_path", type=str, default="")
    p.add_argument("--lora_strength", type=float, default=0.8)
    p.add_argument("--vae_path", type=str, default="")
    p.add_argument("--cond_path", type=str, default="", help="precomputed conditioning tensors (see module docstring)")
    p.add_argument("--synthetic", action="store_true", help="seeded random conditioning + name-keyed synthetic weights")
    p.add_argument("--video_path", type=str, default="", help="directory of frame images, .gif or Motion-JPEG .avi: source of `keyframes`")
    p.add_argument("--prompt_listpath", type=str, default="")
    p.add_argument("--video_listpath", type=str, default="")
    p.add_argument("--videos_directory", type=str, default="", help="directory containing videos to be processed")
    p.add_argument("--json_path", type=str, default="", help="path to json file containing video paths and captions")
    p.add_argument("--videos_root", type=str, default="", help="path to the root of videos")
    p.add_argument("--depth_root", type=str, default="",
                   help="(not in the reference script, whose conditioner runs MiDaS / ZoeDepth itself) directory of <video name>.pt raw "
                        "depth tensors (N, h, w) over all frames of a video; default: <video_path>.depth.pt next to the video")
    p.add_argument("--detect_ratio", type=float, default=1.0)
    p.add_argument("--batch_size", type=int, default=4)
    p.add_argument("--original_fps", type=int, default=20)
    p.add_argument("--target_fps", type=int, default=3)
    p.add_argument("--save_type", type=str, default="npy", choices=["npy", "gif", "mp4", "mjpeg", "png"],
                   help="reference: gif | mp4 (default mp4).  mp4 needs a codec library (none offline: raises, as decoding does); npy = raw frames; "
                        "mjpeg (not in the reference script) = true-colour Motion-JPEG in an .avi, baseline JPEG frames encoded on the GPU "
                        "(ccedit_amd/mjpeg.py, csrc/mjpeg.hip) at --video_quality; H and W must be multiples of 16; png (not in the reference script) = "
                        "lossless true-colour animated PNG, one file per clip, rows filtered and deflate-coded on the GPU (ccedit_amd/png.py, "
                        "csrc/png.hip), any H and W")
    p.add_argument("--video_quality", type=int, default=90,
                   help="(not in the reference script) JPEG quality of --save_type mjpeg, 1 ... 100: the Annex K tables scaled by the usual rule")
    p.add_argument("--save_path", type=str, default="outputs/demo/tv2v")
    p.add_argument("--H", type=int, default=256)
    p.add_argument("--W", type=int, default=384)
    p.add_argument("--num_keyframes", type=int, default=9)
    p.add_argument("--prompt", type=str, default="")
    p.add_argument("--negative_prompt", type=str, default="ugly, low quality")
    p.add_argument("--add_prompt", type=str, default="masterpiece, high quality")
    p.add_argument("--tokenizer_path", type=str, default="",
                   help="directory with the CLIP tokenizer files (vocab.json, merges.txt) of openai/clip-vit-large-patch14: with it "
                        "--prompt / --negative_prompt / --add_prompt are tokenised here as in the reference script; without it the "
                        "conditioning tensors must carry token ids or embeddings (--cond_path)")
    p.add_argument("--prompt_chunks", type=int, default=1, choices=[1, 2, 3, 4],
                   help="(not in the reference script, which truncates at 75 tokens) the largest number of 77-token chunks a prompt may use, "
                        "1 ... 4: a longer prompt is cut into chunks (after a comma where one is near, or at the word BREAK), every chunk is "
                        "encoded on its own and the network sees a context of 77 n rows (ccedit_amd/prompt.py).  A prompt that needs more "
                        "chunks is refused, never truncated.  Applies to every prompt of the run.  1 (default): the path as before")
    p.add_argument("--prompt_syntax", type=str, default="plain", choices=["plain", "weighted"],
                   help="(not in the reference script) weighted: (x) multiplies the emphasis of x by 1.1, [x] divides it by 1.1, (x:1.3) sets "
                        "a factor in [0, 8], nesting multiplies, a backslash before a bracket or a backslash makes it a literal; the weights "
                        "act on the text encoder's output (csrc/prompt.hip).  plain (default): brackets are text, as before")
    p.add_argument("--sample_steps", type=int, default=50)
    p.add_argument("--sampler_name", type=str, default="EulerEDMSampler")       # the reference script's default
    p.add_argument("--discretization_name", type=str, default="LegacyDDPMDiscretization")
    p.add_argument("--cfg_scale", type=float, default=7.5)
    p.add_argument("--prior_coefficient_x", type=float, default=0.0)
    p.add_argument("--prior_coefficient_noise", type=float, default=1.0)
    p.add_argument("--sdedit_denoise_strength", type=float, default=0.0)
    p.add_argument("--inpainting_mode", action="store_true",
                   help="region-restricted editing: only where the clip's mask is white is generated, the rest is re-injected from the "
                        "original before every sampler step (the samplers' sample_inpainting).  Needs a mask: --mask_path, --mask_root "
                        "or <video stem>.mask.png / .mask.gif / .mask/ next to the video")
    p.add_argument("--mask_path", type=str, default="",
                   help="(not in the reference script, which leaves the mask to the user) the edit mask of a single-clip invocation: one "
                        "image for all frames, or a directory of images / a .gif with one mask per frame of the video.  White = edit, black = keep")
    p.add_argument("--mask_root", type=str, default="",
                   help="directory of masks of a multi-clip invocation: <video name>.png, <video name>.gif or <video name>/")
    p.add_argument("--mask_composite", action="store_true",
                   help="with --inpainting_mode: put the original pixels back outside the mask after decoding (the VAE round trip is lossy)")
    p.add_argument("--mask_track", action="store_true",
                   help="(not in the reference script) the mask is ONE image painted on source frame --mask_frame; every frame of the video "
                        "gets its own mask, tracked forwards and backwards along the source's motion on the device (ccedit_amd/masktrack.py, "
                        "csrc/masktrack.hip).  Needs --inpainting_mode and --H, --W multiples of 64")
    p.add_argument("--mask_frame", type=int, default=0, help="with --mask_track: the source frame the mask was painted on")
    p.add_argument("--mask_dilate", type=int, default=0,
                   help="grow every mask (tracked or not) by this many pixels, 0 ... 32: a (2R + 1) x (2R + 1) square maximum, after tracking")
    p.add_argument("--mask_invert", action="store_true",
                   help="swap edit and keep (255 - mask), after tracking and --mask_dilate: with --mask_track, edit everything but the subject")
    p.add_argument("--mask_graded", action="store_true",
                   help="(not in the reference script) the mask's grey levels are edit STRENGTHS: luminance g edits with strength g / 255 "
                        "(white = all the way, as before; mid grey = held to the source for the first half of the schedule, free afterwards; "
                        "black = kept), no cut at 128 (ccedit_amd/softmask.py, csrc/softmask.hip).  Needs --inpainting_mode; not with --mask_track")
    p.add_argument("--mask_feather", type=int, default=0,
                   help="(not in the reference script) soften the mask's edge over this many pixels, 0 ... 64: the mean over a (2R + 1) x (2R + 1) "
                        "square, after --mask_dilate and --mask_invert; whatever mask the run has (painted, tracked, automatic) becomes a "
                        "graded one.  Needs --inpainting_mode")
    p.add_argument("--mask_auto", action="store_true",
                   help="(not in the reference script) no painted mask: the edit mask is computed from --source_prompt (what the video shows) and "
                        "--prompt (what it should show) — the noised source latent is evaluated under both prompts and the mask is where the "
                        "two predictions disagree, cleaned by a vote over space and time (ccedit_amd/automask.py, csrc/automask.hip).  Needs "
                        "--inpainting_mode, --source_prompt and a video with a prompt; costs --mask_auto_samples network evaluations per clip")
    p.add_argument("--source_prompt", type=str, default="", help="with --mask_auto: the prompt that describes the SOURCE video (\"a brown horse\")")
    p.add_argument("--mask_auto_samples", type=int, default=4, help="noise samples of the difference map, 1 ... 16: one network evaluation each")
    p.add_argument("--mask_auto_strength", type=float, default=0.5,
                   help="noise level of the samples, in (0, 1]: the first sigma of the schedule --sdedit_denoise_strength of this value starts from")
    p.add_argument("--mask_auto_quantile", type=float, default=0.99,
                   help="the difference map of a clip is scaled by this quantile of its cells, in [0, 1] (below 1: a few outliers do not set the scale)")
    p.add_argument("--mask_auto_threshold", type=float, default=0.5, help="a cell is set where its difference exceeds this fraction of the scale")
    p.add_argument("--mask_auto_vote", type=int, default=14,
                   help="a cell stays set where at least this many of the 27 cells around it — 3 x 3 in space, one frame either way in time — are "
                        "set, 1 ... 27 (default 14, a majority: specks and one-frame flicker go); 0 = no vote")
    p.add_argument("--mask_auto_seed", type=int, default=None, help="seed of the automatic mask's own noise generator (default: --seed)")
    p.add_argument("--mask_auto_save", type=str, default="",
                   help="directory: the final masks are written to <dir>/<video name>/%%05d.png, one per SOURCE frame (every frame gets its nearest "
                        "keyframe's mask), a sequence --mask_root <dir> accepts as it is — compute once, retouch, reuse (then without "
                        "--mask_dilate / --mask_invert, which the saved masks already hold)")
    p.add_argument("--window_frames", type=int, default=0,
                   help="(not in the reference script) keyframes per network evaluation; with --num_keyframes above it the clip is covered "
                        "by overlapping windows of this many frames whose denoised latents are fused at every sampler evaluation "
                        "(17 for the shipped checkpoints).  0 = off: one window of --num_keyframes frames, as before")
    p.add_argument("--window_overlap", type=int, default=None,
                   help="(not in the reference script) frames shared by consecutive windows, 0 ... window_frames - 1 (default: window_frames // 2)")
    p.add_argument("--tile_h", type=int, default=0,
                   help="(not in the reference script) height in pixels (a multiple of 64) of the tile the network evaluates; with --tile_w, "
                        "a frame with --H above it or --W above --tile_w is covered by overlapping tiles of this size whose denoised latents "
                        "are fused at every sampler evaluation (512 for the shipped checkpoints).  0 = off: the frame as one piece, as before")
    p.add_argument("--tile_w", type=int, default=0,
                   help="(not in the reference script) width in pixels (a multiple of 64) of the tile, see --tile_h (768 for the shipped checkpoints)")
    p.add_argument("--tile_overlap", type=int, default=None,
                   help="(not in the reference script) pixels (a multiple of 8, less than the tile) shared by neighbouring tiles, on both axes "
                        "(default: a quarter of the tile per axis, rounded down to a multiple of 8)")
    p.add_argument("--region_prompt", action="append", default=None,
                   help="(not in the reference script) the prompt of a masked region of the frame; repeatable, region r is the r-th "
                        "--region_prompt / --region_mask pair, 1 ... 7 of them.  --prompt stays the base prompt and covers what the regions "
                        "leave.  Every sampler evaluation runs the network once per prompt and fuses the results (ccedit_amd/regions.py)")
    p.add_argument("--region_mask", action="append", default=None,
                   help="the mask of a region, what --mask_path accepts: one image, a .gif / .png sequence or a directory with one mask per "
                        "frame of the video.  White = this region's prompt.  --mask_dilate / --mask_invert do not apply")
    p.add_argument("--region_feather", type=int, default=1,
                   help="latent cells (8 pixels each), 0 ... 8, over which the blend between regions is feathered (default 1; 0 = a hard split)")
    p.add_argument("--region_track", action="store_true",
                   help="every --region_mask is ONE image painted on source frame --region_frame and followed through the clip on the device "
                        "(ccedit_amd/masktrack.py), like --mask_track.  Needs a video and --H, --W multiples of 64")
    p.add_argument("--region_frame", type=int, default=0, help="with --region_track: the source frame the region masks were painted on")
    p.add_argument("--prompt_at", action="append", default=None, metavar="INDEX:TEXT",
                   help="(not in the reference script) a prompt schedule: from keyframe INDEX (0 ... num_keyframes - 1, negative values count "
                        "from the end, written --prompt_at=-1:TEXT) the prompt is TEXT (everything after the first colon); repeatable.  --prompt stays the base prompt and "
                        "holds from keyframe 0 up to the first keyed index; --add_prompt is put in front of every scheduled text; "
                        "--negative_prompt is not scheduled.  Between two keyed frames the text context moves from one prompt's to the next's "
                        "(--prompt_ease); every frame attends to its own context in ONE network evaluation (ccedit_amd/schedule.py)")
    p.add_argument("--prompt_ease", type=str, default="linear", choices=["linear", "smooth", "step"],
                   help="how the context moves between two keyed frames f0 < f1 of --prompt_at: linear a = (f - f0) / (f1 - f0); smooth "
                        "a^2 (3 - 2 a) of it; step: the earlier prompt before the midpoint, the later one from it on")
    p.add_argument("--propagate", action="store_true",
                   help="(not in the reference script) full-frame-rate output: after a clip's keyframes are saved, every source frame from the "
                        "first to the last keyframe gets an edited frame — the two neighbouring edited keyframes carried along the source's "
                        "motion (ccedit_amd/propagate.py, csrc/propagate.hip) — written to <save_path>/result_full/ at --original_fps.  "
                        "Needs a video source (job mode) and --save_type gif, --save_type mjpeg or --save_type png")
    p.add_argument("--num_samples", type=int, default=1)
    p.add_argument("--noise_seed", type=int, default=None,
                   help="(not in the reference script) draw the samplers' per-step noise from a CPU generator with this seed instead of "
                        "torch.randn_like on the device: the same clip on any GPU / against the CPU oracle (tests)")
    p.add_argument("--noise_warp", action="store_true",
                   help="(not in the reference script) motion-following noise: every noise draw of the run — the start latent, the ancestral "
                        "noise of every step, the re-injection noise of --inpainting_mode, the SDEdit start — is carried from keyframe to "
                        "keyframe along the SOURCE's motion, so that a moving surface keeps its noise; the noise of every single frame stays "
                        "white (ccedit_amd/noisewarp.py, csrc/noisewarp.hip).  Needs --video_path (or its kin) and --H, --W multiples of 64; "
                        "log_info.json gains `noise_warp`")
    p.add_argument("--noise_warp_rho", type=float, default=1.0, action=_StoreGiven,
                   help="with --noise_warp: the correlation of a keyframe's noise with the noise it inherits, 0 ... 1 (default 1: carried "
                        "exactly; below 1 a second, independent draw is mixed in: rho * carried + sqrt(1 - rho^2) * fresh)")
    p.add_argument("--report_quality", action="store_true",
                   help="(not in the reference script) after a clip is saved, measure it on the GPU (ccedit_amd/quality.py, csrc/quality.hip): "
                        "fidelity of the result to the source keyframes (PSNR, SSIM; with --inpainting_mode over the pixels the mask keeps) "
                        "and the warp error of result and source along the source's motion, with the share of pixels the motion estimate "
                        "could follow; with --propagate also over every source frame against result_full/ (`full_rate`).  Written to "
                        "<save_path>/quality/<clip number>.json; log_info.json gains `quality`.  Job mode only.  Measures of fidelity and "
                        "steadiness, not of how well the prompt was followed")
    p.add_argument("--disable_check_repeat", action="store_true")
    p.add_argument("--gpu_io", action="store_true",
                   help="pixel I/O on the GPU (ccedit_amd/csrc/pixel.hip): frame / depth resize, depth hint normalisation and the uint8 "
                        "frames of --save_type gif / mjpeg / png; decoding and file writing stay on the host.  Default off: everything as before")
    p.add_argument("--gif_encoder", type=str, default="pillow", choices=["pillow", "device"],
                   help="(not in the reference script) who encodes the files of --save_type gif, result_full/gif/ of --propagate included.  "
                        "pillow (default): Pillow on the host, byte for byte as before.  device: colour quantisation (Wu's quantiser, a local "
                        "palette of 256 colours per frame) and LZW coding on the GPU (ccedit_amd/gif.py, csrc/gif.hip); with --gpu_io the "
                        "uint8 frames never leave the device, only palettes and LZW bytes come back.  An error with any other --save_type")
    p.add_argument("--gif_decoder", type=str, default="pillow", choices=["pillow", "device"],
                   help="(not in the reference script) who decodes a .gif source (--video_path and its kin; --propagate's source frames).  "
                        "pillow (default): Pillow on the host, as before.  device: LZW decoding and frame compositing on the GPU "
                        "(ccedit_amd/gifdec.py, csrc/gifdec.hip), the same bytes as Pillow's; only the compressed bytes go up; a file outside "
                        "the decoder's subset goes through Pillow with one line on stderr.  Needs --gpu_io; masks stay Pillow's")


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    add_common_args(p)
    return p


def check_args(p: argparse.ArgumentParser, args) -> None:
    """Combinations argparse cannot express: an error exit of the parser itself."""
    if args.mask_composite and not args.inpainting_mode:
        p.error("--mask_composite puts the original back outside the mask of --inpainting_mode: give both")
    if getattr(args, "mask_graded", False) and not args.inpainting_mode:
        p.error("--mask_graded reads the mask of --inpainting_mode as edit strengths: give both")
    if getattr(args, "mask_feather", 0) and not args.inpainting_mode:
        p.error("--mask_feather softens the edge of the mask of --inpainting_mode: give both")
    if args.window_frames < 0:
        p.error("--window_frames must be positive (0 = off)")
    if args.window_overlap is not None and not args.window_frames:
        p.error("--window_overlap is the overlap of the windows of --window_frames: give both")
    if args.window_frames and args.window_overlap is not None and not 0 <= args.window_overlap < args.window_frames:
        p.error("--window_overlap must be in 0 ... window_frames - 1")
    if getattr(args, "tile_h", 0) < 0 or getattr(args, "tile_w", 0) < 0:
        p.error("--tile_h and --tile_w must be positive (0 = off)")
    if bool(getattr(args, "tile_h", 0)) != bool(getattr(args, "tile_w", 0)):
        p.error("--tile_h and --tile_w are the two sides of one tile: give both")
    if getattr(args, "tile_overlap", None) is not None and not getattr(args, "tile_h", 0):
        p.error("--tile_overlap is the overlap of the tiles of --tile_h / --tile_w: give them too")
    if getattr(args, "propagate", False):
        if not job_mode(args):
            p.error("--propagate carries the edit to the frames between the keyframes of a video: give --prompt with --video_path "
                    "(or --prompt_listpath / --videos_directory / --json_path)")
        if args.save_type not in ("gif", "mjpeg", "png"):
            p.error(f"--propagate writes result_full/ as gif, as Motion-JPEG or as animated PNG: add --save_type gif, --save_type mjpeg or "
                    f"--save_type png (got {args.save_type})")
    if getattr(args, "gif_encoder", "pillow") == "device" and args.save_type != "gif":
        p.error(f"--gif_encoder device encodes the files of --save_type gif (got --save_type {args.save_type})")
    if getattr(args, "gif_decoder", "pillow") == "device" and not getattr(args, "gpu_io", False):
        p.error("--gif_decoder device decodes .gif sources where --gpu_io keeps the frames: add --gpu_io")
    if not 1 <= getattr(args, "video_quality", 90) <= 100:
        p.error(f"--video_quality must be in 1 ... 100 (got {args.video_quality})")
    if args.save_type == "mjpeg" and (args.H % 16 or args.W % 16):
        p.error(f"--save_type mjpeg codes 16 x 16 MCUs: --H and --W must be multiples of 16 (got {args.H}x{args.W})")
    check_mask_options(args)                 # (--mask_track and its kin: ValueError, here and again where the masks are made)
    check_region_options(args)               # (--region_prompt and its kin: ValueError; nothing is imported or checked without the flags)
    check_mask_auto(args)                    # (--mask_auto and its kin: ValueError; nothing is imported or checked without the flag)
    check_prompt_schedule(args)              # (--prompt_at: ValueError / NotImplementedError; nothing is imported or checked without the flag)
    check_noise_warp(args)                   # (--noise_warp and its rho: ValueError; nothing is imported without the flag)
    check_report_quality(args)               # (--report_quality: ValueError; nothing is imported without the flag)


def windowing(args) -> bool:
    """Windows are active when the clip has more keyframes than one window holds; otherwise the plain path runs untouched."""
    return getattr(args, "window_frames", 0) > 0 and args.num_keyframes > args.window_frames


def check_windowing(args, with_ref: bool = False) -> None:
    """Before any GPU work: windows cover the TV2V path only (NotImplementedError otherwise)."""
    if not windowing(args):
        return
    if with_ref:
        raise NotImplementedError("--window_frames is not available with a reference image (sampling_tv2v_ref.py): one reference image "
                                  "belongs to the centre frame of one window")
    if args.config_path and os.path.exists(args.config_path):
        from ccedit_amd.windows import check_supported
        with open(args.config_path, "r") as f:
            check_supported(config=f.read())


def tiling(args) -> bool:
    """Tiles are active when both tile flags are set and the frame is larger than the tile on an axis; otherwise the plain path runs untouched."""
    th, tw = getattr(args, "tile_h", 0) or 0, getattr(args, "tile_w", 0) or 0
    return th > 0 and tw > 0 and (args.H > th or args.W > tw)


def tile_overlap_px(args):
    """(rows, columns) of pixels shared by neighbouring tiles: --tile_overlap on both axes, else a quarter of the tile per axis rounded
    down to a multiple of 8."""
    o = getattr(args, "tile_overlap", None)
    return (args.tile_h // 4 // 8 * 8, args.tile_w // 4 // 8 * 8) if o is None else (int(o), int(o))


def tile_plan_args(args):
    """plan2d's arguments (latent units) for the flags: (lh, lw, th, tw, oh, ow)."""
    oh, ow = tile_overlap_px(args)
    return args.H // 8, args.W // 8, args.tile_h // 8, args.tile_w // 8, oh // 8, ow // 8


def first_stage_frames(args) -> int:
    """Frames per first-stage call under tiles: tiles.first_stage_group with T_plain = --window_frames if set, else --num_keyframes."""
    from ccedit_amd.tiles import first_stage_group
    lh, lw, th, tw, _, _ = tile_plan_args(args)
    return first_stage_group(getattr(args, "window_frames", 0) or args.num_keyframes, th, tw, lh, lw)


def check_tiling(args, with_ref: bool = False) -> None:
    """Before any GPU work: what tiles cannot do is refused with what to do instead (ValueError; NotImplementedError for what tiles do
    not cover).  With tiles off everything passes."""
    if not tiling(args):
        return
    th, tw = args.tile_h, args.tile_w
    if th % 64 or tw % 64:
        raise ValueError(f"--tile_h {th} --tile_w {tw}: a tile is evaluated by the network directly, which takes multiples of 64 pixels — "
                         f"choose tile sides that are multiples of 64 (512 x 768 for the shipped checkpoints)")
    oh, ow = tile_overlap_px(args)
    if oh % 8 or ow % 8 or oh < 0 or ow < 0:
        raise ValueError(f"--tile_overlap {oh}: tiles are cut from the latent, 8 pixels per element — give a non-negative multiple of 8")
    if oh >= th or ow >= tw:
        raise ValueError(f"--tile_overlap {max(oh, ow)} is not smaller than the tile ({th}x{tw}): neighbouring tiles must differ — give less")
    if args.H % 8 or args.W % 8:
        raise ValueError(f"--H {args.H} --W {args.W}: tiles are cut from the latent, 8 pixels per element — frame sides must be multiples of 8")
    if args.H < th or args.W < tw:
        raise ValueError(f"--H {args.H} --W {args.W} does not fill one tile of {th}x{tw} on both axes: choose a tile no larger than the frame")
    if with_ref:
        raise NotImplementedError("--tile_h / --tile_w are not available with a reference image (sampling_tv2v_ref.py): the reference "
                                  "latent (`cond_feat`) belongs to the whole frame, not to a tile")
    if getattr(args, "propagate", False) and (args.H % 64 or args.W % 64):
        raise ValueError(f"--propagate with --H {args.H} --W {args.W}: the motion matcher's pyramid (four levels of 8 x 8 blocks) takes frame "
                         f"sides that are multiples of 64 — tiles lift that limit for the network only; choose such a size or drop --propagate")
    from ccedit_amd import tiles
    tiles.plan2d(*tile_plan_args(args))                                            # (more than 64 tiles: its own message)
    tiles.check_frame_cap(args.H // 8, args.W // 8)
    if args.config_path and os.path.exists(args.config_path):
        with open(args.config_path, "r") as f:
            tiles.check_supported(config=f.read())


def first_stage_precision(args) -> str:
    """"fp32" or "bf16", as the engine will set it (ccedit_amd/engine.py): policy vae_fp32 = 1 / 0 decide alone, 2 (the default) follows
    the yaml's `disable_first_stage_autocast`."""
    from ccedit_amd import policy
    v = policy.get("vae_fp32")
    if v != 2:
        return "fp32" if v == 1 else "bf16"
    flag = False
    if args.config_path and os.path.exists(args.config_path):
        from ccedit_amd.config import load_config
        flag = bool(load_config(args.config_path).model.params.get("disable_first_stage_autocast", False))
    return "fp32" if flag else "bf16"


def check_first_stage(args) -> None:
    """Before any GPU work, with tiles or without (the first stage runs on whole frames either way; check_tiling's tiles.check_frame_cap
    bounds its score matrix in both precisions): the bf16 first stage takes fewer latent pixels per frame (vae.check_bf16_frame) and
    would otherwise say so only at decode, after the sampling loop."""
    if args.H % 8 or args.W % 8:
        return                                                                       # (refused where the frames are encoded / decoded)
    from ccedit_amd.vae import check_bf16_frame
    if first_stage_precision(args) == "bf16":
        check_bf16_frame(args.H // 8, args.W // 8)


def check_propagate(args, video_paths) -> None:
    """Before any GPU work: --propagate needs strictly increasing keyframe indices on every clip (ValueError from ccedit_amd.propagate.plan —
    keyframe_indices' linspace fallback on a video that is too short repeats frames).  Clips that cannot be counted here (no decoder)
    are reported where they fail to load, as always."""
    if not getattr(args, "propagate", False):
        return
    from ccedit_amd.propagate import plan
    from scripts.sampling.util import count_video_frames, keyframe_indices
    for v in dict.fromkeys(video_paths):
        video = resolve_video(v)
        if os.path.isdir(video) or (video.endswith((".gif", ".avi")) and os.path.exists(video)):
            n = count_video_frames(video)
            try:
                plan(keyframe_indices(n, args.original_fps, args.target_fps, args.num_keyframes), n)
            except ValueError as e:
                raise ValueError(f"--propagate: {video}: {e}") from e


def video_writer(args):
    """The ONE place that reads --save_type, --gif_encoder and --video_quality -> (the writer's entry in ccedit_amd/video_io.py, None
    where the save type is no movie of uint8 frames (npy); its options: perform_save_locally_video takes them by keyword, the save
    function of scripts/sampling/util.py the entry names by position after fps)."""
    from ccedit_amd.video_io import writer_of
    writer = writer_of(args.save_type, getattr(args, "gif_encoder", "pillow"))
    return writer, {k: getattr(args, k) for k in (writer.options if writer else ())}


def propagate_chunk(args, cvideos, samples, dev, save_path, keep=None):
    """--propagate for one chunk: per clip all source frames on the device, the edited keyframes as the uint8 frames result/ holds
    (frames_to_u8 without rounding of the decoder output), propagate_clip, <save_path>/result_full/gif/animation-XXXX.gif (--save_type
    mjpeg: result_full/mjpeg/animation-XXXX.avi, --save_type png: result_full/png/animation-XXXX.png, encoded from the frames where they
    are, on the device; so is the gif with --gif_encoder device) at --original_fps.  With --mask_composite every in-between frame keeps the source outside ITS OWN mask.  -> the paths written.
    `keep` (a list, --report_quality): per clip (the source frames from the first to the last keyframe, the frames written, their masks or None)
    is appended to it."""
    from ccedit_amd import ops
    from ccedit_amd.propagate import propagate_clip
    from scripts.sampling import util
    from scripts.sampling.util import keyframe_indices, load_video_frames_u8
    writer, options = video_writer(args)
    edited = ops.frames_to_u8(samples.float().contiguous(), rounding=False, unit_range=False)           # (bs, T, H, W, 3)
    paths = []
    for b, v in enumerate(cvideos):
        source = load_video_frames_u8(resolve_video(v), (args.H, args.W), dev, **_gif_decoder(args))
        n_all = source.shape[0]
        masks = None
        if args.inpainting_mode and args.mask_composite:
            masks = all_frame_masks(args, v, n_all, dev)
        idx = keyframe_indices(n_all, args.original_fps, args.target_fps, args.num_keyframes)
        full = propagate_clip(source, idx, edited[b], masks=masks)
        if keep is not None:
            first = int(idx[0])
            keep.append((source[first:first + full.shape[0]], full, None if masks is None else masks[first:first + full.shape[0]]))
        frames = full.contiguous() if writer.on_device else full.cpu().numpy()      # (a device writer encodes the frames where they are)
        save = getattr(util, writer.saver)                                         # (found on the module now: save_gif_u8(path, host frames, fps) for Pillow's gif)
        paths.append(save(os.path.join(save_path, "result_full"), frames, args.original_fps, *options.values()))
    return paths


def parse_args(argv=None):
    p = make_parser()
    args = p.parse_args(argv)
    check_args(p, args)
    return args


def build_model(args):
    from ccedit_amd.utils.synth import fill_module_
    from scripts.sampling.util import create_model
    if not args.config_path:
        raise SystemExit("--config_path is required (e.g. configs/inference_ccedit/keyframe_no2ndca_depthmidas.yaml)")
    dev = torch.device("cuda")
    from scripts.sampling.util import load_lora_file, load_vae_file, model_load_ckpt
    if getattr(args, "tokenizer_path", ""):
        os.environ["CCEDIT_CLIP_TOKENIZER"] = args.tokenizer_path      # read by FrozenCLIPEmbedder when the yaml builds it
    model = create_model(args.config_path, dev)
    if args.ckpt_path:
        model_load_ckpt(model, path=args.ckpt_path)
    elif args.synthetic:
        fill_module_(model.model, prefix="model.")
        fill_module_(model.first_stage_model, prefix="first_stage_model.")
        fill_module_(model.conditioner, prefix="conditioner.")
    else:
        raise SystemExit("need --ckpt_path or --synthetic")
    # sampling_tv2v.py:190-262: optional base-model swap, LoRA merge at --lora_strength, replacement VAE — all weight-space,
    # before the kernels' operands are packed
    if args.basemodel_path:
        model_load_ckpt(model, args.basemodel_path, True)
    if args.lora_path:
        load_lora_file(model, args.lora_path, args.lora_strength)
    if args.vae_path:
        load_vae_file(model, args.vae_path)
    model.pack(dev)
    args.context_dim = model.model.diffusion_model.context_dim     # 768 for the shipped configs
    return model, dev


def conditioning_tensors(args, g: torch.Generator, need_frames: bool, need_ref: bool = False):
    from scripts.sampling.util import load_conditioning
    T = args.num_keyframes
    if args.cond_path:
        cond = load_conditioning(args.cond_path)
    else:
        if args.context_dim == 768:      # shipped configs: seeded random token ids through the CLIP text encoder
            nl = 77 * int(getattr(args, "prompt_chunks", 1) or 1)       # --prompt_chunks N: ids of N chunks
            text = dict(tokens=torch.randint(0, 49406, (1, nl), generator=g), tokens_uc=torch.randint(0, 49406, (1, nl), generator=g))
        else:                            # reduced test configs: a precomputed embedding of the network's context width
            text = dict(crossattn=torch.randn(1, 77, args.context_dim, generator=g),
                        crossattn_uc=torch.randn(1, 77, args.context_dim, generator=g))
        cond = dict(**text,
                    control_hint=(torch.rand(1, 1, T, args.H, args.W, generator=g) * 2 - 1).repeat(1, 3, 1, 1, 1))
        if need_frames:
            cond["keyframes"] = torch.rand(1, 3, T, args.H, args.W, generator=g) * 2 - 1
        if need_ref:
            cond["cond_img"] = torch.rand(1, 3, args.H, args.W, generator=g) * 2 - 1
    if args.video_path:           # sampling_tv2v.py:314-331: keyframes (T,3,H,W) -> (1,3,T,H,W)
        from scripts.sampling.util import load_video_keyframes
        kf = load_video_keyframes(args.video_path, args.original_fps, args.target_fps, T, (args.H, args.W), **_io_device(args, video=True))
        cond["keyframes"] = kf.permute(1, 0, 2, 3)[None].contiguous()
    if need_ref and getattr(args, "reference_path", ""):
        from scripts.sampling.util import load_img
        cond["cond_img"] = load_img(args.reference_path, (args.H, args.W), **_io_device(args))
    for k in (["keyframes"] if need_frames else []) + (["cond_img"] if need_ref else []):
        if k not in cond:
            raise SystemExit(f"--cond_path must hold `{k}` for the requested options")
    return cond


def _gif_decoder(args) -> dict:
    """gif_decoder= of the video loaders: given only with --gif_decoder device (else the loaders' default, the route as before)."""
    return {"gif_decoder": "device"} if getattr(args, "gif_decoder", "pillow") == "device" else {}


def _io_device(args, video: bool = False) -> dict:
    """device= of load_img / load_video_keyframes / load_video_mask: the current GPU under --gpu_io, else nothing (the host route,
    unchanged).  video: a loader of video frames, which takes --gif_decoder through the same dict (masks and images do not)."""
    if not getattr(args, "gpu_io", False):
        return {}
    return dict({"device": torch.device("cuda", torch.cuda.current_device())}, **(_gif_decoder(args) if video else {}))


def text_inputs(cond, dev, args=None):
    """batch['txt'] for prompt / negative prompt: the strings themselves when --tokenizer_path is given (composed as
    sampling_tv2v.py:334-347: add_prompt + ", " + prompt; the negative prompt alone), else token ids (`tokens`, `tokens_uc`:
    (1,77) int64 -> CLIP text encoder on the GPU) or precomputed embeddings (`crossattn`, `crossattn_uc`)."""
    if args is not None and getattr(args, "tokenizer_path", ""):
        prompt = args.add_prompt + ", " + args.prompt if args.add_prompt else args.prompt
        return [prompt], [args.negative_prompt]
    if "tokens" in cond:
        return cond["tokens"].to(dev), cond["tokens_uc"].to(dev)
    return cond["crossattn"].to(dev), cond["crossattn_uc"].to(dev)


# ------------------------------------------------------------------------------------------
# Long and weighted prompts: --prompt_chunks / --prompt_syntax (ccedit_amd/prompt.py)
# ------------------------------------------------------------------------------------------
def prompts_on(args) -> bool:
    """The new text path runs when a flag asks for it; with the defaults (1 chunk, plain) nothing of it is imported or called."""
    return int(getattr(args, "prompt_chunks", 1) or 1) != 1 or getattr(args, "prompt_syntax", "plain") != "plain"


def _text_embedder(model):
    """The conditioner's CLIP embedder (input key `txt`)."""
    for emb in model.conditioner.embedders:
        if getattr(emb, "input_key", None) == "txt" and hasattr(emb, "encode_long"):
            return emb
    raise NotImplementedError("--prompt_chunks / --prompt_syntax: the config has no CLIP text embedder on `txt`")


def compose_prompt(args, q: str) -> str:
    """sampling_tv2v.py:334-347: add_prompt + ", " + prompt."""
    return args.add_prompt + ", " + q if args.add_prompt else q


def warn_truncated(args, model, texts) -> None:
    """The old path (1 chunk, plain, a tokenizer): a prompt whose tokens exceed 75 is truncated as in the reference — one line on
    stderr says so.  Nothing else changes."""
    if prompts_on(args) or not getattr(args, "tokenizer_path", ""):
        return
    tok = _text_embedder(model).tokenizer()
    for t in texts:
        count = len(tok(t, add_special_tokens=False)["input_ids"])
        if count > 75:
            print(f"[prompt] {count} tokens, the text encoder sees 75: the rest of {t[:40]!r}... is dropped — --prompt_chunks "
                  f"{min(-(-count // 75), 4)} keeps it", file=sys.stderr)


def long_text(args, model, dev, full, neg, region=(), source=None):
    """The new text path for one chunk of clips.  `full`, `neg`: the composed prompts and the negative prompts, one per clip; `region`:
    the composed region prompts of the clip.  Every prompt is cut into chunks, all get ONE length 77 n, and the embedder encodes them
    chunk by chunk (weighted: with the emphasis rule).  Returns (txt, txt_uc, [txt of every region], per-clip log entries): txt are
    finished (bs, 77 n, C) embeddings, which the conditioner hands through.  Every refusal is raised before the first launch.
    `source` (--mask_auto): the composed source prompt of the chunk; it takes part in the one length, and its txt, repeated per clip, is
    returned as a FIFTH element (only when `source` is given)."""
    import zlib
    from ccedit_amd import prompt
    prompt.check_options(args.prompt_chunks, args.prompt_syntax)
    weighted = args.prompt_syntax == "weighted"
    names = ([f"--prompt ({i + 1} of {len(full)})" if len(full) > 1 else "--prompt" for i in range(len(full))]
             + [f"--negative_prompt ({i + 1} of {len(neg)})" if len(neg) > 1 else "--negative_prompt" for i in range(len(neg))]
             + [f"--region_prompt {r + 1}" for r in range(len(region))] + (["--source_prompt"] if source is not None else []))
    texts = list(full) + list(neg) + list(region) + ([source] if source is not None else [])
    if args.tokenizer_path:
        emb = _text_embedder(model)
        enc = prompt.encode_prompts(emb.tokenizer(), dict(zip(names, texts)), args.prompt_chunks, args.prompt_syntax)
        n = enc["n"]

        def encode(sel):
            tokens = torch.cat([enc[k]["tokens"] for k in sel]).to(dev)
            weights = torch.cat([enc[k]["weights"] for k in sel]).to(dev) if weighted else None
            return emb.encode_long(tokens, weights)
        counts = {k: (enc[k]["prompt_tokens"], enc[k]["prompt_chunks"]) for k in names}
    else:
        if not args.synthetic:
            raise SystemExit("prompts need --tokenizer_path (vocab.json / merges.txt of openai/clip-vit-large-patch14), or --synthetic")
        n = int(args.prompt_chunks)
        for k, t in zip(names, texts):                       # the grammar is still checked; without a vocabulary there are no weights
            try:
                prompt.parse(t, args.prompt_syntax)
            except ValueError as e:
                raise ValueError(f"{k}: {e}") from None
        by_name = dict(zip(names, texts))

        def encode(sel):
            rows = []
            for k in sel:
                g = torch.Generator().manual_seed(zlib.crc32(by_name[k].encode("utf-8")) & 0x7FFFFFFF)
                if args.context_dim == 768:
                    rows.append(torch.randint(0, 49406, (1, 77 * n), generator=g))
                else:
                    rows.append(torch.randn(1, 77 * n, args.context_dim, generator=g))
            rows = torch.cat(rows).to(dev)
            return _text_embedder(model).encode_long(rows) if args.context_dim == 768 else rows
        counts = {k: (None, n) for k in names}
    nf = len(full)
    txt = encode(names[:nf]) if nf else None
    txt_uc = encode(names[nf:nf + len(neg)]) if neg else None
    region_txt = [encode([k]) for k in names[nf + len(neg):nf + len(neg) + len(region)]]
    log = [dict(prompt_tokens=counts[names[i]][0], prompt_chunks=counts[names[i]][1], negative_prompt_tokens=counts[names[nf + i]][0],
                negative_prompt_chunks=counts[names[nf + i]][1], context_rows=77 * n) for i in range(nf)]
    if source is not None:
        return txt, txt_uc, region_txt, log, encode(["--source_prompt"] * max(nf, 1))
    return txt, txt_uc, region_txt, log


def cond_text(args, model, cond, dev):
    """The text of the tensor mode through the new path when ids of a conditioning file ask for it: `tokens` / `tokens_uc` of (1, 77 n),
    n <= 4, optionally `token_weights` / `token_weights_uc` fp32 of the same shape.  The halves are padded to one n with empty chunks.
    Returns (txt, txt_uc, log entries) or None: the old path."""
    if "tokens" not in cond or getattr(args, "tokenizer_path", ""):
        return None
    long = cond["tokens"].shape[-1] != 77 or cond["tokens_uc"].shape[-1] != 77 or "token_weights" in cond or "token_weights_uc" in cond
    if not (long or prompts_on(args)):
        return None
    from ccedit_amd import prompt
    emb = _text_embedder(model)
    tc, wc = cond["tokens"], cond.get("token_weights")
    tu, wu = cond["tokens_uc"], cond.get("token_weights_uc")
    nc, nu = prompt.check_tokens(tc, wc, "tokens / token_weights"), prompt.check_tokens(tu, wu, "tokens_uc / token_weights_uc")
    n = max(nc, nu)
    bos, eos = emb.special_ids()
    if (wc is None) != (wu is None):                         # one half weighted: the other's tokens all weigh 1
        wc = torch.ones(tc.shape, dtype=torch.float32) if wc is None else wc
        wu = torch.ones(tu.shape, dtype=torch.float32) if wu is None else wu
    tc, wc = prompt.pad_tokens(tc, wc, n, bos, eos)
    tu, wu = prompt.pad_tokens(tu, wu, n, bos, eos)
    txt = emb.encode_long(tc.to(dev), None if wc is None else wc.to(dev))
    txt_uc = emb.encode_long(tu.to(dev), None if wu is None else wu.to(dev))
    return txt, txt_uc, [dict(prompt_tokens=None, prompt_chunks=nc, negative_prompt_tokens=None, negative_prompt_chunks=nu, context_rows=77 * n)]


def save_result(args, tag, x):
    """sampling_tv2v.py:473-515: clamp to [0,1]; .npy frames (default) or an animated gif / a Motion-JPEG .avi / an animated PNG + frame grid."""
    from scripts.sampling.util import perform_save_locally_video, save_frames
    writer, options = video_writer(args)
    if writer and getattr(args, "gpu_io", False):
        perform_save_locally_video(os.path.join(args.save_path, "result"), x, fps=args.target_fps, savetype=args.save_type, gpu_io=True, signed=True,
                                   **options)
    elif writer:
        perform_save_locally_video(os.path.join(args.save_path, "result"), torch.clamp((x + 1.0) / 2.0, 0.0, 1.0),
                                   fps=args.target_fps, savetype=args.save_type, **options)
    save_frames(args.save_path, tag, x)


def _once(first):
    """A noise source whose FIRST draw is the tensor the caller already holds (the start latent's randn, drawn from the run's CPU
    generator as always); whatever is drawn after it is torch.randn_like — the fresh part of --noise_warp_rho < 1."""
    held = [first]
    return lambda x: held.pop() if held else torch.randn_like(x)


def _cpu_noise(sampler, args) -> None:
    """--noise_seed: the ancestral / churn noise (`noise_sampler`, torch.randn_like(x) in the reference: sampling.py:100, 184) from a seeded
    CPU generator, one draw per call in the samplers' own order."""
    seed = getattr(args, "noise_seed", None)
    if seed is not None and hasattr(sampler, "noise_sampler"):
        gen = torch.Generator().manual_seed(int(seed))
        sampler.noise_sampler = lambda x: torch.randn(x.shape, generator=gen).to(x.device)


# ------------------------------------------------------------------------------------------
# Edit masks of --inpainting_mode (white = edit, black = keep the original)
# ------------------------------------------------------------------------------------------
NO_MASK = ("--inpainting_mode needs an edit mask (the reference script stops here too: \"mask should be provided by the user\", "
           "sampling_tv2v.py:385-387).  Looked for: (1) --mask_path, (2) --mask_root/<video name>.png, .gif or --mask_root/<video name>/, "
           "(3) <video stem>.mask.png, <video stem>.mask.gif or <video stem>.mask/ next to the video")


def find_mask(args, video_path: str):
    """The mask of one clip, looked up like its depth (depth_frames): --mask_path, else --mask_root/<video name>.{png,gif} or
    --mask_root/<video name>/, else <video stem>.mask.png | .mask.gif | .mask/.  -> path, or None."""
    if getattr(args, "mask_path", ""):
        return args.mask_path
    if not video_path:
        return None
    stem = video_path[:-4] if video_path.endswith((".mp4", ".gif", ".avi")) else video_path.rstrip("/")
    cands = [(stem + ".mask.png", os.path.isfile), (stem + ".mask.gif", os.path.isfile), (stem + ".mask", os.path.isdir)]
    if getattr(args, "mask_root", ""):
        base = os.path.join(args.mask_root, os.path.basename(stem))
        cands = [(base + ".png", os.path.isfile), (base + ".gif", os.path.isfile), (base, os.path.isdir)] + cands
    for cpath, present in cands:
        if present(cpath):
            return cpath
    return None


def check_mask_options(args) -> None:
    """--mask_track, --mask_frame, --mask_dilate, --mask_invert: what can be refused before a video is opened (ValueError, with what to do)."""
    from ccedit_amd import masktrack
    masktrack.check_dilate(getattr(args, "mask_dilate", 0))
    check_graded(args)
    if not getattr(args, "mask_track", False):
        return
    if not args.inpainting_mode:
        raise ValueError("--mask_track tracks the edit mask of --inpainting_mode: give both")
    masktrack.check_size(args.H, args.W, "--mask_track")
    if getattr(args, "mask_frame", 0) < 0:
        raise ValueError(f"--mask_frame {args.mask_frame} is outside the video: frames count from 0")


def graded_on(args) -> bool:
    """The run is graded — its mask is a map of edit strengths — when --mask_graded or --mask_feather was given; otherwise nothing of
    the graded route is imported or called."""
    return bool(getattr(args, "mask_graded", False) or getattr(args, "mask_feather", 0))


def check_graded(args) -> None:
    """--mask_graded, --mask_feather: what can be refused from the flags alone (ValueError, with what to do).  Without them everything passes."""
    if not graded_on(args):
        return
    from ccedit_amd import softmask
    softmask.check_feather(args.mask_feather)
    if not args.inpainting_mode:
        raise ValueError("--mask_graded / --mask_feather grade the edit mask of --inpainting_mode: give it too")
    if getattr(args, "mask_graded", False) and getattr(args, "mask_track", False):
        raise ValueError("--mask_graded with --mask_track: the tracker follows a BINARY mask through the clip — paint the mask black and "
                         "white and soften the tracked masks with --mask_feather R instead")
    if getattr(args, "propagate", False) and getattr(args, "mask_composite", False):
        raise ValueError("--mask_graded / --mask_feather with --propagate --mask_composite: the frames between the keyframes are composited "
                         "with a binary mask, a soft composite on the keyframes alone would flicker — drop --mask_composite, or drop "
                         "--mask_graded / --mask_feather")
    if _dist_rank_world()[1] > 1:
        raise ValueError("--mask_graded / --mask_feather are not available in the multi-GPU modes (WORLD_SIZE > 1): a graded run is "
                         "evaluated on one GPU — run it with one process")


def finish_masks(args, masks):
    """--mask_dilate, then --mask_invert, then --mask_feather, on the masks of a clip (tracked or not); at the defaults the masks as they
    are, nothing launched."""
    from ccedit_amd import masktrack
    radius, invert = getattr(args, "mask_dilate", 0), getattr(args, "mask_invert", False)
    if radius or invert:
        masks = masktrack.finish(masks.cuda() if not masks.is_cuda else masks, radius, invert)
    feather = getattr(args, "mask_feather", 0)
    if feather:
        from ccedit_amd import ops
        masks = ops.mask_feather((masks.cuda() if not masks.is_cuda else masks).contiguous(), feather)
    return masks


def _graded_kw(args) -> dict:
    """load_video_mask's keyword of --mask_graded: the luminance bytes as they are; without the flag the call as before."""
    return dict(graded=True) if getattr(args, "mask_graded", False) else {}


_TRACKED = {}           # the last clip's tracked masks: --propagate asks for the clip clip_masks has just tracked


def tracked_masks(args, video_path: str, mask_path: str, dev):
    """--mask_track: the ONE mask image `mask_path`, painted on frame --mask_frame, followed through every source frame of the clip
    -> uint8 (F, H, W) on `dev`.  The frames come the way --propagate's do (load_video_frames_u8: the device decoders where they apply)."""
    from ccedit_amd import masktrack, video_io
    from scripts.sampling.util import load_video_frames_u8, load_video_mask
    check_mask_options(args)
    if video_io.kind_of(mask_path, missing_ok=True) is not None:
        raise ValueError(f"--mask_track follows ONE mask image through the clip, but {mask_path} is a mask sequence: give the mask of frame "
                         "--mask_frame as one image, or drop --mask_track to use the sequence as it is")
    if not video_path:
        raise ValueError("--mask_track follows the mask along the source video: give --video_path")
    video = resolve_video(video_path)
    key = (video, mask_path, args.mask_frame, args.H, args.W, str(dev), getattr(args, "gif_decoder", "pillow"))
    if key not in _TRACKED:
        source = load_video_frames_u8(video, (args.H, args.W), dev, **_gif_decoder(args))
        masktrack.chain(source.shape[0], args.mask_frame)                                  # (--mask_frame outside the video: refused here)
        anchor = load_video_mask(mask_path, args.original_fps, args.target_fps, 1, (args.H, args.W), device=dev)[0]
        _TRACKED.clear()
        _TRACKED[key] = masktrack.track_clip(source, anchor.contiguous(), args.mask_frame)
    return _TRACKED[key]


def clip_masks(args, video_paths, dev):
    """The pixel masks of a chunk: uint8 (bs, T, H, W) on `dev`, 0 = keep / 255 = edit, resized like the frames' geometry (nearest).
    A clip without a mask is an error (NotImplementedError, as the flag alone always was).  --mask_track: the keyframes' masks are the
    tracked masks at keyframe_indices; --mask_dilate / --mask_invert apply last."""
    from scripts.sampling.util import count_video_frames, keyframe_indices, load_video_mask
    out = []
    for v in video_paths:
        mpath = find_mask(args, v)
        if mpath is None:
            raise NotImplementedError(f"no mask for {v or 'the clip'}: {NO_MASK}")
        if getattr(args, "mask_track", False):
            full = tracked_masks(args, v, mpath, dev)
            idx = keyframe_indices(full.shape[0], args.original_fps, args.target_fps, args.num_keyframes)
            out.append(finish_masks(args, full[torch.from_numpy(idx.astype("int64")).to(dev)]))
            continue
        video = resolve_video(v) if v else ""
        n_all = count_video_frames(video) if video and (os.path.isdir(video) or video.endswith((".gif", ".avi"))) else None
        out.append(finish_masks(args, load_video_mask(mpath, args.original_fps, args.target_fps, args.num_keyframes, (args.H, args.W), n_all,
                                                      **_io_device(args), **_graded_kw(args))))
    return torch.stack([m.to(dev) for m in out], dim=0).contiguous()


def all_frame_masks(args, video_path: str, n_all: int, dev):
    """clip_masks' sibling for --propagate --mask_composite: the masks of ALL n_all source frames of one clip, uint8 (n_all, H, W) on `dev`
    — the user's sequence, the one image repeated, or with --mask_track the tracked masks; --mask_dilate / --mask_invert apply last."""
    from scripts.sampling.util import load_video_mask
    mpath = find_mask(args, video_path)
    if getattr(args, "mask_track", False):
        return finish_masks(args, tracked_masks(args, video_path, mpath, dev)).contiguous()
    return finish_masks(args, load_video_mask(mpath, args.original_fps, args.target_fps, args.num_keyframes, (args.H, args.W), n_all,
                                              device=dev, all_frames=True, **_graded_kw(args))).contiguous()


# ------------------------------------------------------------------------------------------
# Automatic edit masks: --mask_auto from --source_prompt and --prompt (ccedit_amd/automask.py)
# ------------------------------------------------------------------------------------------
def mask_auto_on(args) -> bool:
    """The automatic mask is active when --mask_auto was given; otherwise nothing of it is imported or called."""
    return bool(getattr(args, "mask_auto", False))


def check_mask_auto(args, with_ref: bool = False) -> None:
    """Before any video is opened, from the flags alone: what --mask_auto needs and what it cannot be combined with (ValueError naming
    the flags, with what to do).  Without the flag everything passes."""
    if not mask_auto_on(args):
        return
    if with_ref:
        raise ValueError("--mask_auto is not available with a reference image (sampling_tv2v_ref.py): the reference image conditions the "
                         "whole frame — compute the mask with sampling_tv2v.py --mask_auto --mask_auto_save DIR and give it as --mask_root DIR")
    if not args.inpainting_mode:
        raise ValueError("--mask_auto computes the edit mask of --inpainting_mode: give both")
    if not getattr(args, "source_prompt", ""):
        raise ValueError("--mask_auto compares the network's prediction under --source_prompt (what the video shows) with the one under "
                         "--prompt (what it should show): give --source_prompt")
    if not job_mode(args):
        raise ValueError("--mask_auto works on a video and its prompt: give --prompt with --video_path (or --prompt_listpath / "
                         "--videos_directory / --json_path)")
    for flag in ("mask_path", "mask_root", "mask_track"):
        if getattr(args, flag, None):
            raise ValueError(f"--mask_auto with --{flag}: two sources for one mask — drop one of them")
    if regions_on(args):
        raise ValueError("--mask_auto with --region_prompt / --region_mask: the automatic mask compares ONE source prompt with ONE target "
                         "prompt — drop one of them")
    if getattr(args, "propagate", False) and getattr(args, "mask_composite", False):
        raise ValueError("--mask_auto with --propagate --mask_composite: compositing the frames between the keyframes needs every source "
                         "frame's mask, the automatic mask has the keyframes' — drop --mask_composite, or save the masks with "
                         "--mask_auto_save DIR and run again with --mask_root DIR")
    if args.H % 8 or args.W % 8:
        raise ValueError(f"--mask_auto with --H {args.H} --W {args.W}: the automatic mask is made per latent cell of 8 x 8 pixels — frame sides must be multiples of 8")
    from ccedit_amd import automask
    automask.check_options(args.mask_auto_samples, args.mask_auto_strength, args.mask_auto_quantile, args.mask_auto_threshold,
                           args.mask_auto_vote)


def mask_auto_seed(args) -> int:
    return int(args.seed if getattr(args, "mask_auto_seed", None) is None else args.mask_auto_seed)


def mask_auto_sigma(args) -> float:
    """The noise level of the automatic mask: the first sigma of the schedule --sdedit_denoise_strength = --mask_auto_strength starts from."""
    from scripts.sampling.util import init_sampling
    sampler = init_sampling(sample_steps=args.sample_steps, sampler_name=args.sampler_name, discretization_name=args.discretization_name,
                            guider_config_target=GUIDER, cfg_scale=args.cfg_scale, img2img_strength=args.mask_auto_strength)
    return float(sampler.discretization(sampler.num_steps)[0])


def _video_name(video_path: str) -> str:
    """<video name> of --mask_root/<video name>/ (find_mask)."""
    stem = video_path[:-4] if video_path.endswith((".mp4", ".gif", ".avi")) else video_path.rstrip("/")
    return os.path.basename(stem)


def save_auto_masks(args, video_path: str, masks) -> str:
    """--mask_auto_save: `masks` uint8 (T, H, W), the final masks of one clip's keyframes -> <dir>/<video name>/%05d.png, one per source
    frame, each frame its nearest keyframe's mask (a tie: the earlier keyframe's).  What --mask_root <dir> reads back.  -> the directory."""
    from PIL import Image
    from ccedit_amd.automask import nearest_keyframe
    from scripts.sampling.util import count_video_frames, keyframe_indices
    n_all = count_video_frames(resolve_video(video_path))
    table = nearest_keyframe(keyframe_indices(n_all, args.original_fps, args.target_fps, args.num_keyframes), n_all)
    out = os.path.join(args.mask_auto_save, _video_name(video_path))
    os.makedirs(out, exist_ok=True)
    host = masks.cpu().numpy()
    for f, k in enumerate(table):
        Image.fromarray(host[k]).save(os.path.join(out, f"{f:05d}.png"))
    return out


def auto_masks(args, model, dev, batch, batch_uc, c, cvideos, keyframes, source_txt):
    """The pixel masks of a chunk from --source_prompt and --prompt, in place of clip_masks: uint8 (bs, T, H, W) on `dev`, 0 = keep /
    255 = edit, --mask_dilate / --mask_invert applied last; and the chunk's part of log_info['mask_auto'].  `source_txt`: batch['txt'] of
    the source prompt, made by the text route of the other prompts.  The conditioning differs from `c` in the text alone (the control
    hint is the same object in both halves); the closure is the one the sampler will get."""
    from ccedit_amd import automask
    bs = keyframes.shape[0]
    for v in cvideos:
        found = find_mask(args, v)
        if found is not None:
            print(f"[automask] {found} is ignored: --mask_auto computes the mask of {v}", file=sys.stderr)
    cs, _ = model.conditioner.get_unconditional_conditioning(dict(batch, txt=source_txt), batch_uc=batch_uc)
    c_src = dict(c, crossattn=cs["crossattn"][:bs].to(dev))
    closure, engine = make_closure(args, model, c)
    gen = automask.generator(mask_auto_seed(args))
    zc = model.first_stage_model.embed_dim
    z = engine.encode_first_stage(keyframes, noise=torch.randn(bs * keyframes.shape[2], zc, args.H // 8, args.W // 8, generator=gen))
    sigma = mask_auto_sigma(args)
    if sigma == 0.0:
        print(f"[automask] --mask_auto_strength {args.mask_auto_strength} of {args.sample_steps} steps starts at sigma 0: the latent is not "
              "noised at all and the difference map comes from one deterministic evaluation — raise --mask_auto_strength or --sample_steps",
              file=sys.stderr)
    acc = automask.AutoMask(closure, wrapper=model.model)(z, sigma, c_src, c, args.mask_auto_samples, gen)
    lat = automask.mask_from(acc, args.mask_auto_quantile, args.mask_auto_threshold, args.mask_auto_vote, names=cvideos, latent=True)
    fractions = lat.float().flatten(1).mean(dim=1).cpu().tolist()
    from ccedit_amd import ops
    px = ops.automask_expand(lat)
    final = torch.stack([finish_masks(args, px[b]) for b in range(bs)], dim=0).contiguous()
    for b, v in enumerate(cvideos):
        if fractions[b] == 0.0:
            print(f"[automask] the mask of {v} is empty: the two prompts' predictions differ nowhere by more than the threshold", file=sys.stderr)
        if getattr(args, "mask_auto_save", ""):
            save_auto_masks(args, v, final[b])
    log = dict(source_prompt=args.source_prompt, samples=int(args.mask_auto_samples), strength=float(args.mask_auto_strength), sigma=sigma,
               quantile=float(args.mask_auto_quantile), threshold=float(args.mask_auto_threshold), vote=int(args.mask_auto_vote),
               seed=mask_auto_seed(args))
    return final, log, [float(f) for f in fractions]


# ------------------------------------------------------------------------------------------
# Prompt schedules: --prompt_at INDEX:TEXT / --prompt_ease (ccedit_amd/schedule.py)
# ------------------------------------------------------------------------------------------
def schedule_on(args) -> bool:
    """A schedule is active when --prompt_at was given; otherwise nothing of it is imported or called."""
    return bool(getattr(args, "prompt_at", None))


def check_prompt_schedule(args, with_ref: bool = False) -> None:
    """Before any video is opened, from the flags alone: what --prompt_at needs and what it cannot be combined with (ValueError /
    NotImplementedError naming the flags).  Without the flag everything passes."""
    if not schedule_on(args):
        return
    if with_ref:
        raise NotImplementedError("--prompt_at is not available with a reference image (sampling_tv2v_ref.py): the reference image belongs "
                                  "to one centre frame, a prompt per time span does not go with it")
    from ccedit_amd import schedule
    schedule.parse(args.prompt_at, args.num_keyframes)               # an index outside the clip, a duplicate, an empty text
    if not (args.prompt and args.video_path) or args.prompt_listpath or args.videos_directory or args.json_path:
        raise ValueError("--prompt_at schedules the prompts of ONE video: give --prompt (the base prompt) with --video_path, not "
                         "--prompt_listpath / --videos_directory / --json_path with their several jobs")
    if regions_on(args):
        raise NotImplementedError("--prompt_at with --region_prompt / --region_mask: region prompts take one context per clip and region — "
                                  "a schedule per region is not implemented, drop one of them")
    if mask_auto_on(args):
        raise NotImplementedError("--prompt_at with --mask_auto: the automatic mask compares ONE source prompt with ONE target prompt — "
                                  "save the mask with --mask_auto_save DIR in a run without --prompt_at and give it as --mask_root DIR")
    if _dist_rank_world()[1] > 1:
        raise NotImplementedError("--prompt_at is not available in the multi-GPU modes (WORLD_SIZE > 1; the frame- and row-sharded network "
                                  "wrappers refuse a text context per frame themselves): a schedule is evaluated on one GPU")


def check_schedule_jobs(args, num_jobs: int) -> None:
    """Before any video is opened: a schedule belongs to ONE clip, so one job per invocation and one clip per chunk (ValueError)."""
    if not schedule_on(args):
        return
    if num_jobs > 1:
        raise ValueError(f"--prompt_at with {num_jobs} jobs: a schedule belongs to one video — run one --prompt / --video_path job per invocation")
    if args.batch_size > 1 and num_jobs * args.num_samples > 1:
        raise ValueError(f"--prompt_at with --batch_size {args.batch_size} and {num_jobs * args.num_samples} clips: a chunk of several clips "
                         "shares one conditioning batch, a schedule belongs to one clip — add --batch_size 1")


def schedule_texts(args):
    """(texts, keys) of the run: the distinct composed-later texts (the base prompt first unless keyframe 0 is keyed) and the keyed
    (keyframe, text id) pairs; ONE text: the schedule says what --prompt alone says, the plain path runs."""
    from ccedit_amd import schedule
    return schedule.distinct(args.prompt, schedule.parse(args.prompt_at, args.num_keyframes))


def schedule_conditioning(args, model, dev, batch, batch_uc, c, uc, txt, keys):
    """The per-frame text contexts of one clip: `txt` holds the P distinct prompts as batch['txt'] takes them (strings, ids or finished
    embeddings); each goes through the conditioner like the main prompt (as a region prompt does), ccedit_prompt_schedule makes the N
    contexts and the negative context is repeated N times — both ONCE per clip.  Returns the log entry; c / uc are updated in place."""
    from ccedit_amd import schedule
    if c["crossattn"].shape[0] != 1:
        raise ValueError(f"--prompt_at with a chunk of {c['crossattn'].shape[0]} clips: a schedule belongs to one clip — add --batch_size 1")
    ctxs = [c["crossattn"][:1]]
    for p in range(1, len(txt)):
        cp, _ = model.conditioner.get_unconditional_conditioning(dict(batch, txt=txt[p:p + 1]), batch_uc=batch_uc)
        ctxs.append(cp["crossattn"][:1].to(dev))
    k0, k1, a = table = schedule.plan(keys, args.num_keyframes, args.prompt_ease)
    c["crossattn"], uc["crossattn"] = schedule.conditioning(torch.cat(ctxs).float().contiguous(), uc["crossattn"][:1], table)
    return schedule.table_log(keys, k0, k1, a, args.prompt_ease)


# ------------------------------------------------------------------------------------------
# Region prompts: --region_prompt / --region_mask pairs (ccedit_amd/regions.py)
# ------------------------------------------------------------------------------------------
def regions_on(args) -> bool:
    """Regions are active when a region flag was given; otherwise the plain path runs untouched (no import, no launch)."""
    return bool(getattr(args, "region_prompt", None) or getattr(args, "region_mask", None))


def check_region_options(args, with_ref: bool = False) -> None:
    """Before any GPU work, from the flags alone: what regions cannot do is refused with what to do instead (ValueError;
    NotImplementedError with a reference image).  Without region flags everything passes."""
    if not regions_on(args):
        return
    if with_ref:
        raise NotImplementedError("--region_prompt / --region_mask are not available with a reference image (sampling_tv2v_ref.py): the "
                                  "reference image conditions the whole frame, not a region")
    from ccedit_amd import regions
    prompts, masks = list(args.region_prompt or []), list(args.region_mask or [])
    regions.check_counts(len(prompts), len(masks))
    regions.check_feather(args.region_feather)
    if args.H % 8 or args.W % 8:
        raise ValueError(f"--H {args.H} --W {args.W}: region masks are counted per latent cell of 8 x 8 pixels — frame sides must be multiples of 8")
    for m in masks:
        if not os.path.exists(m):
            raise ValueError(f"--region_mask {m} does not exist: give one image, a .gif / .png sequence or a directory of masks per region")
    if getattr(args, "region_track", False):
        from ccedit_amd import masktrack, video_io
        masktrack.check_size(args.H, args.W, "--region_track")
        if args.region_frame < 0:
            raise ValueError(f"--region_frame {args.region_frame} is outside the video: frames count from 0")
        for m in masks:
            if video_io.kind_of(m, missing_ok=True) is not None:
                raise ValueError(f"--region_track follows ONE mask image per region through the clip, but {m} is a mask sequence: give the "
                                 "mask of frame --region_frame as one image, or drop --region_track to use the sequence as it is")
        if not (args.video_path or args.video_listpath or args.videos_directory or args.json_path):
            raise ValueError("--region_track follows the region masks along the source video: give --video_path")


def check_region_jobs(args, num_jobs: int) -> None:
    """Before any GPU work: region masks belong to ONE video, so one job per invocation and one clip per chunk (ValueError)."""
    if not regions_on(args):
        return
    if num_jobs > 1:
        raise ValueError(f"--region_prompt / --region_mask with {num_jobs} jobs: region masks belong to one video — run one --prompt / "
                         "--video_path job per invocation")
    if args.batch_size > 1 and num_jobs * args.num_samples > 1:
        raise ValueError(f"--region_prompt / --region_mask with --batch_size {args.batch_size} and {num_jobs * args.num_samples} clips: a chunk "
                         "of several clips shares one conditioning batch, region masks belong to one clip — add --batch_size 1")


def region_pixel_masks(args, video_path: str, dev):
    """The K region masks of the clip -> uint8 (K, T, H, W) on `dev`, 0 / 255, with the keyframe index rule and nearest resize of the edit
    mask (load_video_mask); --region_track: each ONE image painted on --region_frame, tracked through all source frames (the refusals
    of --mask_track), the keyframes' masks taken at keyframe_indices.  --mask_dilate / --mask_invert do not apply."""
    from scripts.sampling.util import count_video_frames, keyframe_indices, load_video_frames_u8, load_video_mask
    check_region_options(args)
    video = resolve_video(video_path) if video_path else ""
    out = []
    if getattr(args, "region_track", False):
        from ccedit_amd import masktrack
        if not video:
            raise ValueError("--region_track follows the region masks along the source video: give --video_path")
        source = load_video_frames_u8(video, (args.H, args.W), dev, **_gif_decoder(args))
        masktrack.chain(source.shape[0], args.region_frame)                              # (--region_frame outside the video: refused here)
        idx = keyframe_indices(source.shape[0], args.original_fps, args.target_fps, args.num_keyframes)
        idx = torch.from_numpy(idx.astype("int64")).to(dev)
        for m in args.region_mask:
            anchor = load_video_mask(m, args.original_fps, args.target_fps, 1, (args.H, args.W), device=dev)[0]
            out.append(masktrack.track_clip(source, anchor.contiguous(), args.region_frame)[idx])
    else:
        n_all = count_video_frames(video) if video and (os.path.isdir(video) or video.endswith((".gif", ".avi"))) else None
        for m in args.region_mask:
            out.append(load_video_mask(m, args.original_fps, args.target_fps, args.num_keyframes, (args.H, args.W), n_all, **_io_device(args)))
    return torch.stack([m.to(dev) for m in out], dim=0).contiguous()


def region_setup(args, model, dev, batch, batch_uc, c, video_path: str, region_txt=None) -> dict:
    """regions= of sample_one for one clip: {} without region flags, else the K + 1 conditional contexts (the base prompt's first; the
    region prompts through job_text and the conditioner like the main prompt) and the device table of blend coefficients."""
    if not regions_on(args):
        return {}
    from ccedit_amd import regions
    if c["crossattn"].shape[0] != 1:
        raise ValueError(f"--region_prompt / --region_mask with a chunk of {c['crossattn'].shape[0]} clips: region masks belong to one clip — "
                         "add --batch_size 1")
    contexts = [c["crossattn"]]
    for r, q in enumerate(args.region_prompt):               # (region_txt: long_text's, one length for all the clip's prompts)
        txt = region_txt[r] if region_txt is not None else job_text(args, [q], dev, args.context_dim)[0]
        cr, _ = model.conditioner.get_unconditional_conditioning(dict(batch, txt=txt), batch_uc=batch_uc)
        contexts.append(cr["crossattn"][:1].to(dev))
    coef = regions.weights(region_pixel_masks(args, video_path, dev), args.region_feather)
    return dict(contexts=contexts, coef=coef)


def region_log(args) -> list:
    """log_info.json `regions`: what every region was given."""
    return [dict(prompt=q, mask=m, feather=int(args.region_feather), tracked=bool(getattr(args, "region_track", False)))
            for q, m in zip(args.region_prompt, args.region_mask)]


# ------------------------------------------------------------------------------------------
# Motion-following noise: --noise_warp (ccedit_amd/noisewarp.py)
# ------------------------------------------------------------------------------------------
def noise_warp_on(args) -> bool:
    """Motion-following noise is active when --noise_warp was given; otherwise nothing of it is imported or called."""
    return bool(getattr(args, "noise_warp", False))


def check_noise_warp(args, with_ref: bool = False) -> None:
    """Before any GPU work, from the flags alone: what --noise_warp needs and what it cannot be combined with (ValueError naming the
    flags, with what to do).  Without the flag only a stray --noise_warp_rho is refused."""
    if not noise_warp_on(args):
        if getattr(args, "noise_warp_rho_given", False):
            raise ValueError("--noise_warp_rho is the correlation of --noise_warp's carried noise: give --noise_warp too, or drop it")
        return
    from ccedit_amd import noisewarp
    noisewarp.check_rho(getattr(args, "noise_warp_rho", 1.0))
    if with_ref:
        raise ValueError("--noise_warp is not available with a reference image (sampling_tv2v_ref.py): the reference image pins the centre "
                         "frame, the carried noise belongs to a run of sampling_tv2v.py — run that script, or drop --noise_warp")
    if _dist_rank_world()[1] > 1:
        raise ValueError("--noise_warp is not available in the multi-GPU modes (WORLD_SIZE > 1): the noise map of a clip is built and "
                         "applied on one GPU — run it with one process")
    if not (args.video_path or getattr(args, "video_listpath", "") or args.videos_directory or args.json_path):
        raise ValueError("--noise_warp carries the noise along the motion of a source video: give --video_path (or --video_listpath / "
                         "--videos_directory / --json_path)")
    if args.H % 64 or args.W % 64:
        raise ValueError(f"--noise_warp with --H {args.H} --W {args.W}: the motion matcher's pyramid (four levels of 8 x 8 blocks) takes frame "
                         "sides that are multiples of 64 — choose such a size, or drop --noise_warp")
    noisewarp.check_clip(args.num_keyframes, args.H, args.W)


_WARPED = {}            # the last clip's noise map and shares: the samples of a clip (--num_samples) share one build


def noise_map(args, video_path: str, dev):
    """--noise_warp for one clip: all source frames on the device the way --propagate's come (load_video_frames_u8), the keyframes'
    frame numbers by keyframe_indices -> (src int32 (K, cells) on `dev`, shares per keyframe).  Cached per clip like the tracked masks."""
    from ccedit_amd import noisewarp
    from scripts.sampling.util import keyframe_indices, load_video_frames_u8
    if not video_path:
        raise ValueError("--noise_warp carries the noise along the motion of a source video: this clip has none — give --video_path")
    video = resolve_video(video_path)
    key = (video, args.original_fps, args.target_fps, args.num_keyframes, args.H, args.W, str(dev), getattr(args, "gif_decoder", "pillow"))
    if key not in _WARPED:
        source = load_video_frames_u8(video, (args.H, args.W), dev, **_gif_decoder(args))
        idx = keyframe_indices(source.shape[0], args.original_fps, args.target_fps, args.num_keyframes)
        _WARPED.clear()
        _WARPED[key] = noisewarp.build(source, idx)
    return _WARPED[key]


def noise_maps(args, video_paths, dev):
    """The maps of a chunk -> (src int32 (bs, K, cells) on `dev`, [shares per keyframe] per clip)."""
    built = [noise_map(args, v, dev) for v in video_paths]
    return torch.stack([b[0] for b in built], dim=0).contiguous(), [b[1] for b in built]


# ------------------------------------------------------------------------------------------
# Quality report: --report_quality (ccedit_amd/quality.py)
# ------------------------------------------------------------------------------------------
def report_quality_on(args) -> bool:
    """The report is made when --report_quality was given; otherwise nothing of it is imported or launched."""
    return bool(getattr(args, "report_quality", False))


def check_report_quality(args) -> None:
    """Before any GPU work, from the flags alone: what --report_quality needs (ValueError naming the flags, with what to do)."""
    if not report_quality_on(args):
        return
    if not job_mode(args):
        raise ValueError("--report_quality measures a saved clip against its source video: give --prompt with --video_path (or "
                         "--prompt_listpath / --videos_directory / --json_path)")
    if _dist_rank_world()[1] > 1:
        raise ValueError("--report_quality is not available in the multi-GPU modes (WORLD_SIZE > 1): a clip's report is made on the GPU "
                         "that holds its frames — run it with one process")
    if args.H < 8 or args.W < 8 or args.H % 4 or args.W % 4:
        raise ValueError(f"--report_quality with --H {args.H} --W {args.W}: SSIM takes 8 x 8 windows at stride 4 — frame sides must be "
                         "multiples of 4 and at least 8; choose such a size, or drop --report_quality")


def quality_chunk(args, keyframes, samples, mask_px, keyframes_paths, save_path, full=()):
    """--report_quality for one chunk: per clip the source keyframes and the result as the uint8 frames original/ and result/ hold (one
    frames_to_u8 call for both, propagate_chunk's arguments), ccedit_amd.quality.report — over the pixels the clip's mask keeps with
    --inpainting_mode — and, with --propagate, the same over every source frame against result_full/ (`full`: what propagate_chunk kept).
    -> per clip the summary log_info.json keeps; the whole report goes to <save_path>/quality/<clip number>.json."""
    import json
    import re
    from ccedit_amd import ops, quality
    n = samples.shape[0]
    u8 = ops.frames_to_u8(torch.cat([keyframes.float(), samples.float()], dim=0).contiguous(), rounding=False, unit_range=False)
    out = []
    for b in range(n):
        rep = quality.report(u8[b], u8[n + b], None if mask_px is None else mask_px[b] >= 128)
        if b < len(full):
            source, result, masks = full[b]
            rep["full_rate"] = quality.report(source.contiguous(), result.contiguous(), masks)
        number = re.search(r"(\d+)\.\w+$", os.path.basename(keyframes_paths[b])).group(1)
        os.makedirs(os.path.join(save_path, "quality"), exist_ok=True)
        path = os.path.join(save_path, "quality", f"{number}.json")
        with open(path, "w") as f:
            json.dump(rep, f, indent=4)
        entry = dict(quality.summary(rep), path=path)
        if "full_rate" in rep:
            entry["full_rate"] = quality.summary(rep["full_rate"])
        out.append(entry)
    return out


def make_closure(args, model, c, ref=None, regions=None):
    """The closure `denoiser(input, sigma, cond)` every sampler evaluation of a chunk goes through — plain, windowed (--window_frames),
    tiled (--tile_h / --tile_w), region prompts outermost — and the engine whose first stage works in groups that fit it.  Used by
    sample_latent and by the automatic mask (auto_masks): both evaluate the network the same way.  -> (closure, engine)."""
    def denoiser(inp, sigma, cc):
        return model.denoiser(model.model, inp, sigma, cc)

    if windowing(args):          # N frames through windows of --window_frames: the sampler sees the same closure over the long latent
        from ccedit_amd.windows import GroupedFirstStage, WindowedDenoiser, check_supported
        if ref is not None:
            raise NotImplementedError("--window_frames is not available with a reference image: it belongs to the centre frame of one window")
        check_supported(cond=c)
        if not tiling(args):
            denoiser = WindowedDenoiser(denoiser, args.window_frames, args.window_overlap, wrapper=model.model)
            model = GroupedFirstStage(model, args.window_frames)      # (the closure above keeps the engine itself)

    if tiling(args):             # a frame above the tile size: tiles outside, windows (if any) inside every tile
        from ccedit_amd import tiles
        from ccedit_amd.windows import GroupedFirstStage
        if ref is not None:
            raise NotImplementedError("--tile_h / --tile_w are not available with a reference image: it belongs to the whole frame, not to a tile")
        tiles.check_supported(cond=c)
        _, _, lth, ltw, loh, low = tile_plan_args(args)
        denoiser = tiles.TiledDenoiser(denoiser, (lth, ltw), (loh, low), wrapper=model.model,
                                       window=args.window_frames if windowing(args) else 0, window_overlap=args.window_overlap)
        model = GroupedFirstStage(model, first_stage_frames(args))

    if regions:                  # a prompt per region: the OUTERMOST wrapper, around the plain, the windowed or the tiled closure
        from ccedit_amd.regions import RegionDenoiser
        if ref is not None:
            raise NotImplementedError("--region_prompt / --region_mask are not available with a reference image: it conditions the whole frame")
        denoiser = RegionDenoiser(denoiser, regions["contexts"], regions["coef"], wrapper=model.model)      # (the grouped first stage hands .model on)
    return denoiser, model


def sample_latent(args, model, dev, c, uc, randn, keyframes=None, ref=None, prior_type="video", mask=None, regions=None, noise_src=None):
    """sampling_tv2v.py:361-468 for one chunk: the sampled latent.  `mask`: the uint8 LATENT mask (bs, T, H / 8, W / 8) of
    --inpainting_mode (ops.mask_latent of the pixel masks; 1 = edit) — in a graded run (--mask_graded / --mask_feather) the uint8 latent
    STRENGTHS (ops.mask_latent_graded).  `regions`: region_setup's dict (region prompts), or nothing.  `noise_src`: the chunk's noise
    maps (bs, T, cells) of --noise_warp (noise_maps), or nothing: the start noise and every draw of the sampler go through them."""
    from scripts.sampling.util import init_sampling, prior_latent, sdedit_start
    denoiser, model = make_closure(args, model, c, ref=ref, regions=regions)

    inpaint = getattr(args, "inpainting_mode", False)
    if inpaint and mask is None:
        raise NotImplementedError(NO_MASK)

    def run(sampler, start):
        """What the reference's commented-out branch does with a user's mask (sampling_tv2v.py:395-407, 454-466): the known latent is the
        encoded clip, the loop is the sampler's sample_inpainting (uc['control_hint'] already equals c['control_hint'] here)."""
        if not inpaint:
            return sampler(denoiser, start, c, uc=uc)
        if not hasattr(sampler, "sample_inpainting"):
            raise NotImplementedError(f"{args.sampler_name} has no inpainting loop (the reference has one for the EDM and the ancestral samplers)")
        z = model.encode_first_stage(keyframes)
        if graded_on(args):              # `mask` holds latent STRENGTHS: a cell is re-injected while its strength is below the step's threshold
            return sampler.sample_inpainting(denoiser, start, c, uc=uc, x0=z, strength=mask)
        return sampler.sample_inpainting(denoiser, start, c, uc=uc, x0=z, mask=mask)

    def warp_noise(sampler):
        """--noise_warp: around whatever the noise source is by now (--noise_seed's CPU generator or the device's), so that every draw
        of the walk — ancestral, churn, re-injection — is carried.  -> the source sdedit_start draws from, or None: its own."""
        if noise_src is None:
            return None
        from ccedit_amd import noisewarp
        wrapped = noisewarp.wrap(getattr(sampler, "noise_sampler", torch.randn_like), noise_src, args.noise_warp_rho)
        if hasattr(sampler, "noise_sampler"):
            sampler.noise_sampler = wrapped
        return wrapped

    if args.sdedit_denoise_strength == 0.0:
        if noise_src is not None:            # the start noise is carried like every later draw (at rho < 1 with a fresh part from the device)
            from ccedit_amd import noisewarp
            randn = noisewarp.wrap(_once(randn), noise_src, args.noise_warp_rho)(randn)
        if args.prior_coefficient_x != 0.0:
            randn = prior_latent(model, randn, args.prior_coefficient_x, args.prior_coefficient_noise, keyframes, ref, prior_type)
        sampler = init_sampling(sample_steps=args.sample_steps, sampler_name=args.sampler_name,
                                discretization_name=args.discretization_name, guider_config_target=GUIDER,
                                cfg_scale=args.cfg_scale)
        _cpu_noise(sampler, args)
        warp_noise(sampler)
        return run(sampler, randn)
    else:
        assert 0.0 < args.sdedit_denoise_strength <= 1.0, "sdedit_denoise_strength should be in (0, 1]"
        assert args.prior_coefficient_x == 0, "prior_coefficient_x should be 0 when using sdedit_denoise_strength"
        sampler = init_sampling(sample_steps=args.sample_steps, sampler_name=args.sampler_name,
                                discretization_name=args.discretization_name, guider_config_target=GUIDER,
                                cfg_scale=args.cfg_scale, img2img_strength=args.sdedit_denoise_strength)
        _cpu_noise(sampler, args)
        carried = warp_noise(sampler)
        return run(sampler, sdedit_start(model, sampler, keyframes, **(dict(noise=carried) if carried is not None else {})))


def sample_one(args, model, dev, c, uc, randn, keyframes=None, ref=None, prior_type="video", mask=None, mask_px=None, regions=None,
               noise_src=None):
    """sampling_tv2v.py:361-470 for one chunk: sample, decode and — with --mask_composite and the pixel masks `mask_px` — put the
    original pixels back outside the mask (ccedit_mask_composite; in a graded run in proportion to the pixel strengths,
    ccedit_mask_composite_graded)."""
    extra = dict(regions=regions) if regions else {}
    if noise_src is not None:
        extra["noise_src"] = noise_src
    z = sample_latent(args, model, dev, c, uc, randn, keyframes=keyframes, ref=ref, prior_type=prior_type, mask=mask, **extra)
    if tiling(args) or windowing(args):
        from ccedit_amd.windows import GroupedFirstStage
        model = GroupedFirstStage(model, first_stage_frames(args) if tiling(args) else args.window_frames)
    samples = model.decode_first_stage(z)
    if getattr(args, "mask_composite", False) and mask_px is not None:
        from ccedit_amd import ops
        composite = ops.mask_composite_graded if graded_on(args) else ops.mask_composite
        samples = composite(samples.float().contiguous(), keyframes.float().contiguous(), mask_px)
    return samples


# ------------------------------------------------------------------------------------------
# Job mode: the reference script's list / directory / BalanceCC-json surface (sampling_tv2v.py:106-204, 264-515)
# ------------------------------------------------------------------------------------------
def expand_jobs(args, with_ref: bool = False):
    """The (prompt, video) jobs of one invocation, as the reference expands them — sampling_tv2v.py:106-160, and with `with_ref`
    sampling_tv2v_ref.py:124-194 (one reference image per job: --reference_path, or --reference_root/output-<Target Prompt>.png in the
    json layout, where jobs whose save directory exists are dropped).  Returns (prompts, video_paths, video_save_paths, ref_paths);
    video_save_paths is empty except in the json layout.  Same assertions and messages as the reference."""
    import json
    prompts, video_paths, video_save_paths, ref_paths = [], [], [], []
    assert not (args.prompt_listpath and args.videos_directory), (
        "Only one of prompt_listpath and videos_directory can be provided, "
        "but got prompt_listpath: {}, videos_directory: {}".format(args.prompt_listpath, args.videos_directory))
    if args.prompt_listpath:
        with open(args.prompt_listpath, "r") as f:
            prompts = [q.strip() for q in f.readlines()]
        assert args.video_listpath, (
            "video_listpath must be provided when prompt_listpath is provided, "
            "but got video_listpath: {}".format(args.video_listpath))
        with open(args.video_listpath, "r") as f:
            video_paths = [q.strip() for q in f.readlines()]
    elif args.videos_directory:
        for video_name in sorted(os.listdir(args.videos_directory)):       # (sorted: os.listdir order is arbitrary in the reference)
            video_path = os.path.join(args.videos_directory, video_name)
            if os.path.isdir(video_path):
                prompts.append(video_name)
                video_paths.append(video_path)
    elif args.json_path:
        assert args.videos_root != "", "videos_root must be provided when json_path is provided"
        if with_ref:
            assert getattr(args, "reference_root", "") != "", "reference_root must be provided when json_path is provided"
        with open(args.json_path, "r") as f:
            json_dict = json.load(f)
        for item in json_dict:
            video_path = os.path.join(args.videos_root, item["Video Type"], item["Video Name"] + ".mp4")
            for edit in item["Editing"]:
                video_save_path = os.path.join(args.save_path, item["Video Type"], item["Video Name"], edit["Target Prompt"])
                if with_ref and os.path.exists(video_save_path):           # sampling_tv2v_ref.py:165-167
                    print(f"video {video_save_path} exists, skip it.")
                    continue
                video_paths.append(video_path)
                prompts.append(edit["Target Prompt"])
                video_save_paths.append(video_save_path)
                if with_ref:
                    ref_paths.append(os.path.join(args.reference_root, "output-{}.png".format(edit["Target Prompt"])))
    else:
        assert args.prompt and args.video_path, (
            "prompt and video_path must be provided when prompt_listpath and videos_directory are not provided, "
            "but got prompt: {}, video_path: {}".format(args.prompt, args.video_path))
        prompts, video_paths = [args.prompt], [args.video_path]
    assert len(prompts) == len(video_paths), (
        "The number of prompts and video_paths must be the same, and you provided {} prompts and {} video_paths".format(
            len(prompts), len(video_paths)))
    if with_ref and not args.json_path:
        # sampling_tv2v_ref.py:192-193 keeps ONE reference path whatever the number of jobs (zip then drops all chunks but the first);
        # here the single --reference_path serves every job of the list
        ref_paths = [getattr(args, "reference_path", "")] * len(prompts)
    return prompts, video_paths, video_save_paths, ref_paths


def basemodel_list(args):
    """sampling_tv2v.py:186-204: the base models to loop over ("default" = the checkpoint as loaded)."""
    assert not (args.basemodel_path and args.basemodel_listpath), (
        "Only one of basemodel_path and basemodel_listpath can be provided, "
        "but got basemodel_path: {}, basemodel_listpath: {}".format(args.basemodel_path, args.basemodel_listpath))
    paths = []
    if args.basemodel_listpath:
        with open(args.basemodel_listpath, "r") as f:
            paths = [q.strip() for q in f.readlines()]
    if args.basemodel_path:
        paths = [args.basemodel_path]
    if args.use_default:
        paths = ["default"] + paths
    return paths or ["default"]


def resolve_video(video_path: str) -> str:
    """The json layout names <Video Name>.mp4; without a codec library (none offline) the same clip as a directory of frames
    <Video Name>/, as <Video Name>.gif or as <Video Name>.avi (Motion-JPEG) is taken instead.  Nothing else is rewritten."""
    if video_path.endswith(".mp4"):
        stem = video_path[:-4]
        if os.path.isdir(stem):
            return stem
        if os.path.exists(stem + ".gif"):
            return stem + ".gif"
        if os.path.exists(stem + ".avi"):
            return stem + ".avi"
    return video_path


def depth_frames(args, video_path: str, keyframes: torch.Tensor) -> torch.Tensor:
    """Raw depth (1, 1, T, H, W) of the clip's keyframes.  The reference's conditioner runs MiDaS dpt_hybrid / ZoeDepth on the RGB
    keyframes (encoders/modules.py:1289-1392); those networks are not part of this build, their output enters as data:
    --depth_root/<video name>.pt or <video_path>.depth.pt holding the depth of ALL frames (N, h, w) — the keyframe index rule and a
    bicubic resize are applied here like to the frames (the keyframes are selected first, only they are resized) — or, with
    --synthetic, the keyframes' luminance.  Under --gpu_io the selected raw depth is uploaded and resized by ccedit_resize_f32_bicubic."""
    from scripts.sampling.util import keyframe_indices
    stem = video_path[:-4] if video_path.endswith((".mp4", ".gif", ".avi")) else video_path.rstrip("/")
    cands = ([os.path.join(args.depth_root, os.path.basename(stem) + ".pt")] if args.depth_root else []) + [stem + ".depth.pt"]
    T, H, W = keyframes.shape[2], keyframes.shape[3], keyframes.shape[4]
    for cpath in cands:
        if os.path.exists(cpath):
            d = torch.load(cpath, map_location="cpu").float()
            if d.dim() != 3:
                raise ValueError(f"{cpath}: expected raw depth (N, h, w) over all frames, got {tuple(d.shape)}")
            d = d[keyframe_indices(d.shape[0], args.original_fps, args.target_fps, T)]
            if getattr(args, "gpu_io", False):
                from ccedit_amd import ops
                return ops.resize_bicubic(d[:, None].contiguous().to(keyframes.device), (H, W))[:, 0][None, None]
            d = torch.nn.functional.interpolate(d[:, None], size=(H, W), mode="bicubic", align_corners=False)[:, 0]
            return d[None, None]
    if args.synthetic:
        kf = keyframes.float().cpu()
        return (0.299 * kf[:, 0:1] + 0.587 * kf[:, 1:2] + 0.114 * kf[:, 2:3])
    raise NotImplementedError(
        f"no depth for {video_path}: the depth annotators (MiDaS dpt_hybrid / ZoeDepth, encoders/modules.py:1289-1392) are not part of "
        f"this build — provide {cands[-1]} (raw depth (N, h, w) of all frames) or --depth_root")


def _hint_embedder(model):
    """The conditioner's depth embedder (input key `control_hint`): its normalize_gpu is the kernel route of the normalisation."""
    for emb in model.conditioner.embedders:
        if getattr(emb, "input_key", None) == "control_hint" and hasattr(emb, "normalize_gpu"):
            return emb
    raise NotImplementedError("--gpu_io: the config has no depth embedder on `control_hint`")


def job_text(args, prompts, dev, context_dim: int):
    """batch['txt'] / batch_uc['txt'] of a chunk: strings when --tokenizer_path is given (add_prompt + ", " + prompt, the negative prompt
    bs times: sampling_tv2v.py:339-347); with --synthetic and no tokenizer files, token ids (embeddings at reduced context widths)
    seeded by the text — the same prompt always maps to the same ids."""
    import zlib
    full = [args.add_prompt + ", " + q if args.add_prompt else q for q in prompts]
    neg = [args.negative_prompt for _ in prompts]
    if args.tokenizer_path:
        return full, neg
    if not args.synthetic:
        raise SystemExit("prompts need --tokenizer_path (vocab.json / merges.txt of openai/clip-vit-large-patch14), or --synthetic")

    def one(text):
        g = torch.Generator().manual_seed(zlib.crc32(text.encode("utf-8")) & 0x7FFFFFFF)
        if context_dim == 768:
            return torch.randint(0, 49406, (1, 77), generator=g)
        return torch.randn(1, 77, context_dim, generator=g)
    return torch.cat([one(t) for t in full]).to(dev), torch.cat([one(t) for t in neg]).to(dev)


def _dist_rank_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def run_jobs(args, with_ref: bool = False) -> None:
    """sampling_tv2v.py:106-515 (sampling_tv2v_ref.py with `with_ref`): jobs -> num_samples -> chunks of batch_size -> for every base model,
    for every chunk: keyframes, conditioning, one CFG-doubled batch through the sampler, decode, original / result / control_hint +
    log_info.json."""
    import json
    check_windowing(args, with_ref)
    check_tiling(args, with_ref)
    check_first_stage(args)
    check_region_options(args, with_ref)
    check_mask_auto(args, with_ref)
    check_prompt_schedule(args, with_ref)
    check_noise_warp(args, with_ref)
    check_report_quality(args)
    from ccedit_amd.parallel import shard_clips
    from scripts.sampling.util import chunk, load_img, load_video_keyframes, model_load_ckpt, perform_save_locally_video
    prompts, video_paths, video_save_paths, ref_paths = expand_jobs(args, with_ref)
    num_samples, batch_size = args.num_samples, args.batch_size
    check_propagate(args, video_paths)
    check_region_jobs(args, len(prompts))
    check_schedule_jobs(args, len(prompts))
    sched_texts, sched_keys = schedule_texts(args) if schedule_on(args) else ([], [])
    print("\nNumber of prompts: {}".format(len(prompts)))
    print("Generate {} samples for each prompt".format(num_samples))
    rep = lambda lst: [item for item in lst for _ in range(num_samples)]
    prompts_chunk = list(chunk(rep(prompts), batch_size))
    video_paths_chunk = list(chunk(rep(video_paths), batch_size))
    ref_paths_chunk = list(chunk(rep(ref_paths), batch_size)) if with_ref else [()] * len(prompts_chunk)
    # the json layout saves chunk idx under video_save_paths[idx] (sampling_tv2v.py:483): one job per chunk there
    if video_save_paths:
        assert batch_size == 1 and num_samples == 1, "the json layout saves one job per directory: use --batch_size 1 --num_samples 1"
    rank, world = _dist_rank_world()
    mine = set(shard_clips(len(prompts_chunk), rank, world))              # config 5: independent clips, one stream of chunks per GPU
    basemodels = basemodel_list(args)

    args_nobase = argparse.Namespace(**vars(args))
    args_nobase.basemodel_path = ""
    if world > 1:                                                         # one process per GPU (torch.distributed.run sets LOCAL_RANK)
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % max(torch.cuda.device_count(), 1))
    model, dev = build_model(args_nobase)
    args.context_dim = args_nobase.context_dim
    T, H, W = args.num_keyframes, args.H, args.W
    g = torch.Generator().manual_seed(args.seed + 7919 * rank)
    for basemodel_idx, basemodel_path in enumerate(basemodels):
        print("-> base model idx: ", basemodel_idx)
        print("-> base model path: ", basemodel_path)
        if basemodel_path != "default" and basemodel_path:
            print("--> load a new base model from {}".format(basemodel_path))
            model_load_ckpt(model, basemodel_path, True)
            model.pack(dev)
        base_tag = basemodel_path.split("/")[-1].split(".")[0]
        log_name = "log_info.json" if world == 1 else f"log_info.rank{rank}.json"
        log_path = os.path.join(args.save_path, base_tag, log_name)
        if os.path.exists(log_path):
            with open(log_path, "r") as f:
                log_info = json.load(f)
        else:
            log_info = {"basemodel_path": basemodel_path, "lora_path": args.lora_path, "vae_path": args.vae_path,
                        "video_paths": [], "keyframes_paths": []}
        for idx, (cprompts, cvideos, crefs) in enumerate(zip(prompts_chunk, video_paths_chunk, ref_paths_chunk)):
            if idx not in mine:
                continue
            cprompts, cvideos, crefs = list(cprompts), list(cvideos), list(crefs)
            if not args.disable_check_repeat:                            # sampling_tv2v.py:297-309: leading videos already done are dropped
                while cvideos and cvideos[0] in log_info["video_paths"]:
                    print(f"video [{cvideos[0]}] has been processed, skip it.")
                    cprompts.pop(0)
                    cvideos.pop(0)
                    if crefs:
                        crefs.pop(0)
                if not cvideos:
                    continue
            bs = min(len(cprompts), batch_size)
            print(f"\nProgress: {idx} / {len(prompts_chunk)}. ")
            try:
                kfs = [load_video_keyframes(resolve_video(v), args.original_fps, args.target_fps, T, (H, W), **_io_device(args, video=True)).permute(1, 0, 2, 3)[None]
                       for v in cvideos]
            except Exception as e:                                       # (:312-330: a clip that does not load is reported and skipped)
                print(f"Error when loading video from  {cvideos}: {type(e).__name__}: {e}")
                continue
            keyframes = torch.cat(kfs, dim=0).to(dev)                    # (bs, 3, T, H, W) in [-1, 1]
            depth = torch.cat([depth_frames(args, v, k) for v, k in zip(cvideos, kfs)], dim=0).to(dev)
            region_txt = prompt_log = source_txt = sched_log = None
            if len(sched_texts) > 1:         # a prompt schedule: its P distinct texts ride as P "clips" through the text route of the flags
                cprompts = list(sched_texts)
            if prompts_on(args):     # every prompt of the chunk in chunks of 77 tokens, one length for all (refusals before any launch)
                source_kw = dict(source=compose_prompt(args, args.source_prompt)) if mask_auto_on(args) else {}
                txt, txt_uc, region_txt, prompt_log, *source_txt = long_text(args, model, dev, [compose_prompt(args, q) for q in cprompts],
                                                                             [args.negative_prompt for _ in cprompts],
                                                                             [compose_prompt(args, q) for q in (args.region_prompt or [])],
                                                                             **source_kw)
                source_txt = source_txt[0] if source_txt else None
            else:
                txt, txt_uc = job_text(args, cprompts, dev, args.context_dim)
                warn_truncated(args, model, txt + txt_uc[:1] if args.tokenizer_path else [])
                if mask_auto_on(args):          # the source prompt through the same route: add_prompt, the tokenizer or --synthetic's seeded ids
                    source_txt = job_text(args, [args.source_prompt] * len(cprompts), dev, args.context_dim)[0]
                    warn_truncated(args, model, source_txt[:1] if args.tokenizer_path else [])
            if args.gpu_io:          # raw depth -> finished hint by the kernels; the embedder passes a finished hint through
                depth = _hint_embedder(model).normalize_gpu(depth)
            batch = {"txt": txt, "control_hint": depth}
            batch_uc = {"txt": txt_uc, "control_hint": depth.clone()}     # uc keeps the SAME hint (:339-344)
            ref = None
            if with_ref:
                if getattr(args, "auto_ref_editing", False):
                    print("Conduct auto ref editing, args.reference_path is ignored.")
                    raise NotImplementedError                            # as the reference: sampling_tv2v_ref.py:366-369
                ref = torch.cat([load_img(r, (H, W), **_io_device(args)) for r in crefs], dim=0).to(dev)
                batch["cond_img"], batch_uc["cond_img"] = ref, ref.clone()
            if len(sched_texts) > 1:         # (the conditioner sees one clip: the base text's; the others follow in schedule_conditioning)
                batch["txt"], batch_uc["txt"] = txt[:1], txt_uc[:1]
            c, uc = model.conditioner.get_unconditional_conditioning(batch, batch_uc=batch_uc)
            for k in c:
                if isinstance(c[k], torch.Tensor):
                    c[k], uc[k] = c[k][:bs].to(dev), uc[k][:bs].to(dev)
            if len(sched_texts) > 1:
                sched_log = schedule_conditioning(args, model, dev, batch, batch_uc, c, uc, txt, sched_keys)
            elif schedule_on(args):          # every keyed text is the base prompt: the plain path, logged
                from ccedit_amd import schedule
                sched_log = schedule.table_log(sched_keys, *schedule.plan(sched_keys, args.num_keyframes, args.prompt_ease), args.prompt_ease)
            randn = torch.randn(bs, 4, T, H // 8, W // 8, generator=g).to(dev)
            mask_px = mask_lat = auto_log = None
            if args.inpainting_mode:                                      # (no mask: NotImplementedError, as the flag alone always was)
                from ccedit_amd import ops
                if mask_auto_on(args):                                    # the mask from the two prompts, in place of clip_masks
                    mask_px, auto_log, auto_fractions = auto_masks(args, model, dev, batch, batch_uc, c, cvideos, keyframes, source_txt)
                else:
                    mask_px = clip_masks(args, cvideos, dev)
                mask_lat = ops.mask_latent_graded(mask_px) if graded_on(args) else ops.mask_latent(mask_px)
            region_kw = dict(regions=region_setup(args, model, dev, batch, batch_uc, c, cvideos[0], region_txt)) if regions_on(args) else {}
            warp_shares = None
            if noise_warp_on(args):                                       # one map per clip of the chunk, built once per clip
                region_kw["noise_src"], warp_shares = noise_maps(args, cvideos, dev)
            t0 = time.time()
            samples = sample_one(args, model, dev, c, uc, randn, keyframes=keyframes, ref=ref,
                                 prior_type=getattr(args, "prior_type", "video"), mask=mask_lat, mask_px=mask_px, **region_kw)
            torch.cuda.synchronize()
            print(f"chunk {idx}: {bs} clip(s) of {T} frames {H}x{W} in {time.time() - t0:.2f}s")
            to01 = lambda v: (torch.clamp(v.float(), -1.0, 1.0) + 1.0) / 2.0
            save_path = video_save_paths[idx] if video_save_paths else os.path.join(args.save_path, base_tag)
            writer, io = video_writer(args)
            if args.gpu_io and writer:                                    # uint8 frames made on the device: clamp((x + 1) / 2) is in the kernel
                to01, io = (lambda v: v), dict(io, gpu_io=True, signed=True)          # (.npy keeps fp32 frames: the host route)
            perform_save_locally_video(os.path.join(save_path, "original"), to01(keyframes), args.target_fps, args.save_type, save_grid=False, **io)
            keyframes_paths = perform_save_locally_video(os.path.join(save_path, "result"), to01(samples), args.target_fps, args.save_type,
                                                         return_savepaths=True, save_grid=False, **io)
            perform_save_locally_video(os.path.join(save_path, "control_hint"), to01(c["control_hint"]), args.target_fps, args.save_type,
                                       save_grid=False, **io)
            if mask_px is not None:                                       # the mask as it was applied, same naming as control_hint/
                m01 = (mask_px >= 128).float()[:, None].expand(-1, 3, -1, -1, -1).contiguous()
                if graded_on(args):                                       # grey images: the writers' uint8(255 v) of (g + 0.5) / 255 is the byte g
                    m01 = ((mask_px.float() + 0.5) / 255.0)[:, None].expand(-1, 3, -1, -1, -1).contiguous()
                perform_save_locally_video(os.path.join(save_path, "mask"), m01 * 2.0 - 1.0 if io.get("signed") else m01, args.target_fps, args.save_type,
                                           save_grid=False, **io)
            full_kept = [] if report_quality_on(args) else None
            if args.propagate:
                log_info.setdefault("fullrate_paths", [])
                log_info["fullrate_paths"] += propagate_chunk(args, cvideos, samples, dev, save_path, keep=full_kept)
            if report_quality_on(args):                                   # measured on the frames just saved; no step code runs
                log_info.setdefault("quality", [])
                log_info["quality"] += quality_chunk(args, keyframes, samples, mask_px, keyframes_paths, save_path, full_kept)
            print("Saved samples to {}. Enjoy.".format(save_path))
            log_info["video_paths"] += cvideos
            log_info["keyframes_paths"] += keyframes_paths
            if regions_on(args):
                log_info["regions"] = region_log(args)
            if prompt_log is not None:
                log_info.setdefault("prompts", [])
                log_info["prompts"] += prompt_log
            if sched_log is not None:
                log_info["prompt_schedule"] = sched_log
            if graded_on(args):
                log_info["mask_graded"], log_info["mask_feather"] = bool(args.mask_graded), int(args.mask_feather)
            if warp_shares is not None:                                   # rho once; per clip the share of cells of every keyframe that inherit
                log_info["noise_warp"] = dict(rho=float(args.noise_warp_rho), inherited=warp_shares[-1],       # (the clip done last; all of them:)
                                              clips=log_info.get("noise_warp", {}).get("clips", []) + warp_shares)
            if auto_log is not None:                                      # the settings once, the fraction of latent cells set per clip
                log_info["mask_auto"] = dict(auto_log, fractions=log_info.get("mask_auto", {}).get("fractions", []) + auto_fractions)
            os.makedirs(os.path.dirname(log_path), exist_ok=True)
            for out in {log_path, os.path.join(save_path, log_name)}:    # (the reference writes it under save_path; the loop reads it per base model)
                os.makedirs(os.path.dirname(out), exist_ok=True)
                with open(out, "w") as f:
                    json.dump(log_info, f, indent=4)
        if basemodel_idx + 1 < len(basemodels) and basemodel_path != "default":
            print("--> back to the original model: {}".format(args.ckpt_path))
            model, dev = build_model(args_nobase)                        # (:517-520: the checkpoint is loaded again before the next base model)


def single_clip_masks(args, dev) -> dict:
    """mask= / mask_px= of sample_one for the single-clip (tensor) mode: {} without --inpainting_mode."""
    if not args.inpainting_mode:
        return {}
    from ccedit_amd import ops
    mask_px = clip_masks(args, [args.video_path], dev)
    return dict(mask=ops.mask_latent_graded(mask_px) if graded_on(args) else ops.mask_latent(mask_px), mask_px=mask_px)


def job_mode(args) -> bool:
    return bool(args.prompt_listpath or args.videos_directory or args.json_path or (args.prompt and args.video_path))


def main():
    args = parse_args()
    torch.manual_seed(args.seed)
    torch.set_grad_enabled(False)
    if job_mode(args):
        return run_jobs(args)
    check_windowing(args)
    check_tiling(args)
    check_first_stage(args)
    check_region_jobs(args, 1)
    check_noise_warp(args)
    from scripts.sampling.util import ResumeLog, save_frames
    model, dev = build_model(args)
    T, h, w = args.num_keyframes, args.H // 8, args.W // 8
    g = torch.Generator().manual_seed(args.seed)
    need_frames = args.prior_coefficient_x != 0.0 or args.sdedit_denoise_strength != 0.0 or args.inpainting_mode
    masks = single_clip_masks(args, dev)
    cond = conditioning_tensors(args, g, need_frames)
    hint = cond["control_hint"].to(dev)
    region_txt = prompt_log = None
    if prompts_on(args) and args.tokenizer_path:
        txt, txt_uc, region_txt, prompt_log = long_text(args, model, dev, [compose_prompt(args, args.prompt)], [args.negative_prompt],
                                                        [compose_prompt(args, q) for q in (args.region_prompt or [])])
    else:
        long = cond_text(args, model, cond, dev)         # ids of (1, 77 n) from --cond_path or --synthetic; None: the path as before
        if long is None:
            txt, txt_uc = text_inputs(cond, dev, args)
            warn_truncated(args, model, txt + txt_uc if args.tokenizer_path else [])
        else:
            txt, txt_uc, prompt_log = long
            if regions_on(args):
                if txt.shape[1] != 77 * args.prompt_chunks:
                    raise ValueError(f"--region_prompt with ids of {txt.shape[1] // 77} chunks: the region prompts get --prompt_chunks "
                                     f"{args.prompt_chunks} chunks here — all contexts of a clip need one length")
                region_txt = long_text(args, model, dev, [], [], [compose_prompt(args, q) for q in args.region_prompt])[2]
    batch = {"txt": txt, "control_hint": hint}
    batch_uc = {"txt": txt_uc, "control_hint": hint.clone()}                              # uc keeps the SAME hint (:339-344)
    c, uc = model.conditioner.get_unconditional_conditioning(batch, batch_uc=batch_uc)
    keyframes = cond["keyframes"].to(dev) if need_frames else None
    if regions_on(args):
        masks["regions"] = region_setup(args, model, dev, batch, batch_uc, c, args.video_path, region_txt)
    warp_shares = None
    if noise_warp_on(args):
        masks["noise_src"], warp_shares = noise_maps(args, [args.video_path], dev)
    log = ResumeLog(args.save_path)
    for i in range(args.num_samples):
        tag = f"sample_{i:04d}"
        if log.done(tag) and not args.disable_check_repeat:
            continue
        randn = torch.randn(1, 4, T, h, w, generator=g).to(dev)                           # CPU generator, like :363
        t0 = time.time()
        x = sample_one(args, model, dev, c, uc, randn, keyframes=keyframes, **masks)
        torch.cuda.synchronize()
        save_result(args, tag, x)
        print(f"{tag}: {T} frames {args.H}x{args.W} in {time.time() - t0:.2f}s")
        if regions_on(args):
            log.log["regions"] = region_log(args)
        if prompt_log is not None:
            log.log["prompts"] = prompt_log
        if warp_shares is not None:
            log.log["noise_warp"] = dict(rho=float(args.noise_warp_rho), inherited=warp_shares[0])
        log.add(tag)


if __name__ == "__main__":
    main()
