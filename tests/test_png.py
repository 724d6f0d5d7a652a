"""Lossless PNG / APNG output, the part that needs no GPU (ccedit_amd/png.py, --save_type png, tests/_png_numpy.py).

The numpy restatement — the definition the kernels of csrc/png.hip equal byte for byte (tests/test_png_gpu.py) — against independent
decoders: zlib inflates every stream to the filtered bytes, an un-filter written from the PNG specification gives the frame back, Pillow
opens the files.  Crafted byte streams and histograms take every path of the deflate stages (each case asserts that it did).  The
container, the command-line surface, APNG as a source, the C ABI, the plain C++ of csrc/png_huff.h under the host's sanitizers, and the
file sizes against Pillow's default PNG."""
import io
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _png_cases as K  # noqa: E402
import _png_numpy as M  # noqa: E402
from ccedit_amd import png as P  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def parse_png(data: bytes):
    """-> [(type, payload)] with every CRC checked."""
    assert data[:8] == P.SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + payload) & 0xffffffff, kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def pillow_frames(path):
    im = Image.open(path)
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.array(im.convert("RGB")))
    return im, np.stack(out, axis=0)


def pillow_png_bytes(frame) -> int:
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    return len(buf.getvalue())


# ---- round trips and the container -----------------------------------------------------------------
@pytest.mark.parametrize("h,w", K.SMALL_SHAPES + list(K.BORDER_SHAPES.values()))
def test_stream_round_trip(h, w):
    for k, kind in enumerate(K.CONTENTS if h * w <= 64 * 96 else ["photo", "checker"]):
        frame = K.frame(kind, h, w, k)
        filtered = M.filter_frame(frame)
        assert filtered.shape == (h, P.row_bytes(w)) and filtered[:, 0].max() < P.FILTERS
        stream = M.zlib_stream(filtered.tobytes())
        assert stream[:2] == b"\x78\x01"
        assert zlib.decompress(stream) == filtered.tobytes()
        assert (M.unfilter(filtered.tobytes(), h, w) == frame).all()


def test_filter_rule():
    """The minimum-sum rule, ties to the lowest number, the zero row above the first."""
    flat = K.frame("flat", 4, 5)
    f = M.filter_frame(flat)
    assert f[0, 0] == 1 and f[1:, 0].tolist() == [2, 2, 2]                # Sub beats None on row 0 (Up = None there); Up is all zeros below
    zero = np.zeros((3, 4, 3), np.uint8)
    assert M.filter_frame(zero)[:, 0].tolist() == [0, 0, 0]               # every filter costs 0: the lowest number
    ramp = K.frame("ramp", 33, 50)
    x = ramp.reshape(33, 150).astype(int)
    f = M.filter_frame(ramp)
    for y in (0, 7, 32):                                                  # the chosen filter's bytes are what the specification says
        t = f[y, 0]
        a = np.concatenate([np.zeros(3, int), x[y, :-3]])
        b = x[y - 1] if y else np.zeros(150, int)
        want = {0: x[y], 1: x[y] - a, 2: x[y] - b, 3: x[y] - (a + b) // 2}.get(int(t))
        if want is not None:
            assert (f[y, 1:] == (want & 255)).all()


@pytest.mark.parametrize("h,w,n", [(17, 19, 3), (64, 96, 5), (33, 50, 2)])
def test_apng_file(tmp_path, h, w, n):
    frames = K.clip(h, w, n)
    path = M.write_apng(str(tmp_path / "a.png"), frames, 143)
    chunks = parse_png(open(path, "rb").read())
    kinds = [k for k, _ in chunks]
    assert kinds == [b"IHDR", b"acTL"] + [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    assert chunks[1][1] == struct.pack(">II", n, 0)
    seq = [struct.unpack(">I", p[:4])[0] for k, p in chunks if k in (b"fcTL", b"fdAT")]
    assert seq == list(range(2 * n - 1))                                   # fcTL and fdAT share one sequence
    for k, p in chunks:
        if k == b"fcTL":
            assert struct.unpack(">IIIIIHHBB", p)[1:] == (w, h, 0, 0, 143, 1000, 0, 0)
    streams = [p for k, p in chunks if k == b"IDAT"] + [p[4:] for k, p in chunks if k == b"fdAT"]
    for s, f in zip(streams, frames):
        assert zlib.decompress(s) == M.filter_frame(f).tobytes()
    im, got = pillow_frames(path)
    assert im.n_frames == n and im.info["duration"] == 143.0 and (got == frames).all()


def test_one_frame_is_a_plain_png(tmp_path):
    frames = K.clip(17, 19, 1)
    path = M.write_apng(str(tmp_path / "one.png"), frames, 50)
    assert [k for k, _ in parse_png(open(path, "rb").read())] == [b"IHDR", b"IDAT", b"IEND"]
    im, got = pillow_frames(path)
    assert getattr(im, "n_frames", 1) == 1 and (got == frames).all()


def test_write_apng_refuses():
    with pytest.raises(ValueError, match="no frames"):
        P.write_apng("x.png", [], 50, 4, 4)
    with pytest.raises(ValueError, match="duration"):
        P.write_apng("x.png", [b"\x78\x01\x03\x00\x00\x00\x00\x01"], 70000, 4, 4)
    with pytest.raises(ValueError, match="zlib stream"):
        P.write_apng("x.png", [b"\x78"], 50, 4, 4)
    for h, w in ((0, 4), (4, 0), (65536, 1), (4096, 4097)):
        with pytest.raises(ValueError):
            P.check_size(h, w)
    P.check_size(4096, 4096)
    assert not os.path.exists("x.png")


# ---- crafted byte streams for the deflate stages ---------------------------------------------------
def _spans(tok):
    """-> [(position, length, distance or 0)] of a chunk's tokens."""
    out, at = [], 0
    for t in tok.tolist():
        if t & P.TOKEN_MATCH:
            n, d = ((t >> 16) & 255) + 3, (t & 0xffff) + 1
        else:
            n, d = 1, 0
        out.append((at, n, d))
        at += n
    return out


@pytest.mark.parametrize("name", sorted(K.streams()))
def test_crafted_streams_inflate(name):
    data = K.streams()[name]
    chunks, stream = K.stream_reference(name)
    assert zlib.decompress(stream) == data and len(chunks) == P.chunks_of(len(data))
    for (tok, hist, blk, bits), part in zip(chunks, M.split(data)):
        assert sum(n for _, n, _ in _spans(tok)) == len(part)               # no token leaves its chunk
        assert all(d <= at for at, _, d in _spans(tok))                     # no match reaches before the chunk's first byte
        assert (M.histogram_of(tok) == hist).all() and bits.n == blk.bits <= P.SLOT_BYTES * 8
        assert blk.header.n <= P.HEADER_MAX_BITS
        assert M.kraft(blk.lit_len, P.MAX_BITS) == 1 << P.MAX_BITS and M.kraft(blk.cl_len, P.CL_MAX_BITS) == 1 << P.CL_MAX_BITS
        used = sum(1 for v in blk.dist_len if v)
        assert M.kraft(blk.dist_len, P.MAX_BITS) == (1 << P.MAX_BITS if used > 1 else (1 << P.MAX_BITS - 1) * used)


def test_crafted_paths_are_taken():
    (tok, hist, blk, _), = K.stream_reference("run")[0]                     # one repeated byte
    assert _spans(tok) == [(0, 1, 0), (1, 258, 1), (259, 258, 1), (517, 5, 1)]
    assert hist[285] == 2 and blk.lit_len[285] and [s for s in range(30) if blk.dist_len[s]] == [0] and blk.dist_len[0] == 1
    (tok, hist, blk, _), = K.stream_reference("norepeat")[0]                # no three-byte repeat: no distance code
    assert len(tok) == 256 and not (tok & P.TOKEN_MATCH).any() and not any(blk.dist_len) and blk.hdist == 1
    (tok, hist, blk, _), = K.stream_reference("single")[0]                  # one byte: two literal/length symbols
    assert [s for s in range(286) if blk.lit_len[s]] == [7, 256] and blk.lit_len[7] == blk.lit_len[256] == 1
    (tok, _, _, _), = K.stream_reference("two")[0]
    assert tok.tolist() == [7, 9]
    (tok, _, _, _), = K.stream_reference("distances")[0]                    # distances 1, 2, 3, 4
    assert [d for _, _, d in _spans(tok) if d] == [1, 2, 3, 4]
    (tok, _, blk, _), = K.stream_reference("far")[0]                        # the largest distance that leaves three bytes
    assert _spans(tok)[-1] == (P.CHUNK - 3, 3, P.CHUNK - 3) and blk.dist_len[M.dist_symbol(P.CHUNK - 3)[0]]
    first, second = K.stream_reference("past_end")[0]                       # a run over the border: the match is cut by the chunk's end
    last = _spans(first[0])[-1]
    assert last[0] + last[1] == P.CHUNK and last[1] == (P.CHUNK - 1) % 258 and last[2] == 1
    assert _spans(second[0])[:2] == [(0, 1, 0), (1, 99, 1)]                 # and the next chunk starts from an empty table
    noise = K.stream_reference("noise")[0]
    assert len(noise) == 3 and len(noise[2][0]) == 1                        # 2 CHUNK + 1 bytes: the last chunk holds one byte


def test_length_limits_are_reached():
    """Fibonacci counts: the unlimited tree is deeper than 15 (7 for the code-length alphabet); the lengths sent are within the limit
    and complete, and zlib inflates the block."""
    tok, hist = K.token_cases()["fibonacci"]
    blk = M.Block(hist, True)
    assert blk.lit_unlimited > P.MAX_BITS and max(blk.lit_len) == P.MAX_BITS and M.kraft(blk.lit_len, P.MAX_BITS) == 1 << P.MAX_BITS
    assert len(tok) < P.CHUNK and not any(blk.dist_len)
    data = K.literal_bytes(tok)
    assert zlib.decompress(b"\x78\x01" + blk.emit(tok).tobytes() + struct.pack(">I", zlib.adler32(data))) == data
    tok, hist = K.token_cases()["codelengths"]
    blk = M.Block(hist, True)
    assert blk.cl_unlimited > P.CL_MAX_BITS and max(blk.cl_len) == P.CL_MAX_BITS and M.kraft(blk.cl_len, P.CL_MAX_BITS) == 1 << P.CL_MAX_BITS
    assert len(tok) < P.CHUNK
    data = K.literal_bytes(tok)
    assert zlib.decompress(b"\x78\x01" + blk.emit(tok).tobytes() + struct.pack(">I", zlib.adler32(data))) == data


def test_code_lengths_properties():
    rs = np.random.RandomState(3)
    for trial in range(200):
        n = int(rs.randint(2, 287))
        counts = np.zeros(286, int)
        counts[rs.choice(286, n, replace=False)] = (rs.pareto(0.6, n) * 3 + 1).astype(int).clip(1, 1 << 20)
        for max_bits in (15, 9):
            if n > 1 << max_bits:
                continue
            lengths, unlimited = M.code_lengths(counts, max_bits)
            assert M.kraft(lengths, max_bits) == 1 << max_bits and max(lengths) <= max_bits
            assert [bool(v) for v in lengths] == [bool(c) for c in counts]
            if unlimited <= max_bits:                                      # then it IS the Huffman code: optimal, so no longer than a flat code
                assert sum(c * l for c, l in zip(counts, lengths)) <= counts.sum() * int(np.ceil(np.log2(n)))
    assert M.code_lengths([0, 0, 5, 0], 15) == ([0, 0, 1, 0], 1) and M.code_lengths([0] * 4, 15) == ([0] * 4, 0)


def test_symbol_tables():
    for length in range(3, 259):
        s, eb, ev = M.length_symbol(length)
        assert P.LEN_BASE[s - 257] + ev == length and ev < 1 << eb and eb == P.LEN_EXTRA[s - 257]
    assert M.length_symbol(258) == (285, 0, 0) and M.length_symbol(257)[0] == 284
    for d in list(range(1, 600)) + [P.CHUNK - 3, P.CHUNK, 32768]:
        s, eb, ev = M.dist_symbol(d)
        assert P.DIST_BASE[s] + ev == d and ev < 1 << eb
    assert P.HEADER_WORDS == 144 and P.SLOT_BYTES % 16 == 0 and P.SLOT_BYTES * 8 >= P.HEADER_MAX_BITS + 16 * P.CHUNK + 15
    assert 8192 <= P.CHUNK <= 32768 and P.CHUNK < 0xffff


# ---- the plain C++ of the kernels under the host's sanitizers ---------------------------------------
def _case(f, final, data, tok, hist, blk, bits):
    f.write(struct.pack("<ii", 0 if data is not None else 1, int(final)))
    if data is not None:
        f.write(struct.pack("<i", len(data)) + data + struct.pack("<i", len(tok)) + tok.astype("<u4").tobytes())
    f.write(np.asarray(hist).astype("<u4").tobytes() + blk.code_table().astype("<u4").tobytes() + struct.pack("<i", blk.header.n)
            + blk.header_words().astype("<u4").tobytes() + struct.pack("<iii", blk.bits, blk.lit_unlimited, blk.dist_unlimited))
    if data is not None:
        raw = bits.tobytes()
        f.write(struct.pack("<i", len(raw)) + raw)


def test_png_huff_hardening(tmp_path):
    """csrc/png_huff.h — the LZ77 walk, the code construction, the header, a token's bits: the text the kernels run — compiled for the
    host with AddressSanitizer and UBSan, over every crafted stream (each chunk in a buffer of exactly its size), the crafted
    histograms and 40 random ones: every word equals the restatement, nothing is read or written out of bounds, exit 0."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "png_huff_harden")
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libsan" if clang else "-static-libasan"]
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san, os.path.join(ROOT, "tests", "png_huff_harden.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    cases = str(tmp_path / "cases.bin")
    count = 0
    with open(cases, "wb") as f:
        f.write(b"PNH1" + struct.pack("<i", 0))
        for name in sorted(K.streams()):
            chunks = K.stream_reference(name)[0]
            for k, ((tok, hist, blk, bits), part) in enumerate(zip(chunks, M.split(K.streams()[name]))):
                _case(f, k == len(chunks) - 1, part, tok, hist, blk, bits)
                count += 1
        for name, (tok, hist) in sorted(K.token_cases().items()):
            _case(f, True, None, tok, hist, M.Block(hist, True), None)
            count += 1
        rs = np.random.RandomState(5)
        for trial in range(40):
            hist = np.zeros(P.HIST_WORDS, np.uint32)
            n = int(rs.randint(1, 286))
            hist[rs.choice(286, n, replace=False)] = (rs.pareto(0.5, n) * 2 + 1).astype(np.int64).clip(1, 60000)
            hist[P.EOB] = 1
            nd = int(rs.randint(0, 31))
            hist[P.DIST_AT + rs.choice(30, nd, replace=False)] = (rs.pareto(0.5, nd) * 2 + 1).astype(np.int64).clip(1, 60000)
            _case(f, trial % 2, None, None, hist, M.Block(hist, trial % 2), None)
            count += 1
        f.seek(4)
        f.write(struct.pack("<i", count))
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert f"{count} cases, 0 mismatches" in run.stdout, run.stdout


# ---- host logic ------------------------------------------------------------------------------------
def test_flags():
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    p = S.make_parser()
    assert p.parse_args(["--save_type", "png"]).save_type == "png"          # not a choice before this format existed
    S.check_args(p, p.parse_args(["--save_type", "png", "--H", "17", "--W", "19", "--video_quality", "50"]))      # any H and W
    with pytest.raises(SystemExit):
        S.check_args(p, p.parse_args(["--gif_encoder", "device", "--save_type", "png"]))
    a = S.parse_args(["--propagate", "--save_type", "png", "--prompt", "a fox", "--video_path", "clips/fox"])
    assert a.propagate and a.save_type == "png"
    assert R.parse_args(["--propagate", "--save_type", "png", "--prompt", "a fox", "--video_path", "clips/fox"]).save_type == "png"


def test_save_level_refusals(tmp_path):
    import torch
    from scripts.sampling.util import perform_save_locally_video
    with pytest.raises(ValueError, match="savetype must be 'gif'"):
        perform_save_locally_video(str(tmp_path), torch.zeros(1, 3, 2, 8, 8), 3, "png", gif_encoder="device")
    with pytest.raises(ValueError, match="gpu_io saves uint8 frames"):
        perform_save_locally_video(str(tmp_path), torch.zeros(1, 3, 2, 8, 8), 3, "png", gpu_io=True)
    assert not os.listdir(str(tmp_path))
    for bad in (np.zeros((1, 8, 8, 3), np.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="on the device"):
            P.encode_frames(bad)


def test_frames_per_launch_follows_the_scratch_bound(monkeypatch):
    assert P.frames_per_launch(17, 19) == P.MAX_FRAMES_PER_LAUNCH
    full = P.frames_per_launch(512, 768)
    assert 1 <= full <= P.MAX_FRAMES_PER_LAUNCH
    monkeypatch.setattr(P, "SCRATCH_BYTES", 1)
    assert P.frames_per_launch(512, 768) == 1


def test_apng_is_a_source_and_a_still_png_is_what_it_was(tmp_path):
    import torch
    from scripts.sampling import util as U
    frames = K.clip(33, 50, 5)
    apng = M.write_apng(str(tmp_path / "clip.png"), frames, 50)
    still = str(tmp_path / "still.png")
    Image.fromarray(frames[0]).save(still)
    assert U.count_video_frames(apng) == 5
    got = U.load_video_keyframes(apng, 20, 20, 3)                           # the host route of a .gif: frames 0, 1, 2 in [-1, 1]
    want = torch.from_numpy(frames[:3]).permute(0, 3, 1, 2).float() / 255.0 * 2.0 - 1.0
    assert got.shape == (3, 3, 33, 50) and torch.equal(got, torch.clamp(want, -1.0, 1.0))
    # a still .png: not a video, as before
    for fn in (lambda: U.count_video_frames(still), lambda: U.load_video_keyframes(still, 20, 20, 3)):
        with pytest.raises(ValueError, match="Unsupported video format"):
            fn()
    # masks: an animated .png holds one mask per frame, a still one serves every keyframe (as before)
    ms = (np.random.RandomState(0).rand(5, 33, 50) > 0.5).astype(np.uint8) * 255
    mask_apng = M.write_apng(str(tmp_path / "mask.png"), np.repeat(ms[..., None], 3, axis=3), 50)
    got = U.load_video_mask(mask_apng, 20, 20, 3, num_allframes=5)
    assert got.shape == (3, 33, 50) and (got.numpy() == ms[:3]).all()
    with pytest.raises(ValueError, match="has 5 frames"):
        U.load_video_mask(mask_apng, 20, 20, 3, num_allframes=6)
    Image.fromarray(ms[1]).save(still)
    got = U.load_video_mask(still, 20, 20, 3, num_allframes=6)
    assert got.shape == (3, 33, 50) and all((g.numpy() == ms[1]).all() for g in got)


# ---- the C ABI: header, exports and binding agree (the conventions of tests/test_cabi.py) ------------
def test_cabi_png():
    import ctypes
    from ccedit_amd import hip
    from ccedit_amd.csrc.build import build
    lib = ctypes.CDLL(build(force=False, verbose=False))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccedit_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ccedit_[a-z0-9_]+)\s*\(", src)) if n.startswith("ccedit_png_"))
    assert declared == ["ccedit_png_adler", "ccedit_png_chunk_bytes", "ccedit_png_codes", "ccedit_png_emit", "ccedit_png_filter", "ccedit_png_pack",
                        "ccedit_png_pack_scan", "ccedit_png_slot_bytes", "ccedit_png_tokens"]
    for n in declared:
        assert hasattr(lib, n) and n in hip.EXPORTS
        args = re.search(re.escape(n) + r"\s*\(([^)]*)\)", src).group(1)
        assert len(hip._SIGS[n][1]) == (0 if args.strip() == "void" else len(args.split(","))), n
    assert "#define CCEDIT_ABI_VERSION 12" in src and hip.ABI_VERSION == 12
    l = hip.lib()                                              # argument validation runs before any HIP call
    assert l.ccedit_png_slot_bytes() == P.SLOT_BYTES and l.ccedit_png_chunk_bytes() == P.CHUNK
    assert l.ccedit_png_filter(None, 16, 1, 8, 8, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_filter(16, 16, 0, 8, 8, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_png_filter(16, 16, 1, 4096, 4097, None) == -1 and b"2^24" in l.ccedit_last_error()
    assert l.ccedit_png_filter(16, 16, 1, 0, 8, None) == -1 and l.ccedit_png_filter(16, 16, 1, 1, 65536, None) == -1
    assert l.ccedit_png_tokens(16, 16, None, 16, 1, 100, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_tokens(16, 16, 16, 16, 0, 100, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_png_tokens(16, 16, 16, 16, 1, 0, None) == -1 and b"L=0" in l.ccedit_last_error()
    assert l.ccedit_png_tokens(16, 16, 16, 16, 1, 1 << 26, None) == -1
    assert l.ccedit_png_tokens(16, 18, 16, 16, 1, 100, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_png_tokens(16, 16, 16, 16, 60000, 1 << 24, None) == -1 and b"2^22 chunks" in l.ccedit_last_error()
    assert l.ccedit_png_codes(16, 16, 16, 16, None, 1, 1, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_codes(16, 16, 16, 16, 16, 0, 1, None) == -1 and b"N=0" in l.ccedit_last_error()
    assert l.ccedit_png_codes(16, 16, 16, 16, 16, 1, 0, None) == -1 and b"C=0" in l.ccedit_last_error()
    assert l.ccedit_png_codes(16, 16, 16, 18, 16, 1, 1, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_png_emit(16, 16, 16, 16, 16, None, 1, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_emit(16, 16, 16, 16, 16, 16, 0, None) == -1 and b"chunks=0" in l.ccedit_last_error()
    assert l.ccedit_png_emit(16, 16, 16, 16, 16, 18, 1, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_png_pack_scan(16, 16, None, 1, 1, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_pack_scan(16, 12, 16, 1, 1, None) == -1 and b"aligned" in l.ccedit_last_error()
    assert l.ccedit_png_pack_scan(16, 16, 16, 70000, 1, None) == -1 and b"N=70000" in l.ccedit_last_error()
    assert l.ccedit_png_pack(16, 16, 16, None, 1, 1, 10, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_pack(16, 16, 16, 16, 1, 1, 0, None) == -1 and b"out_bytes=0" in l.ccedit_last_error()
    assert l.ccedit_png_pack(16, 16, 16, 16, 1, 1 << 23, 10, None) == -1
    assert l.ccedit_png_adler(16, None, 16, 1, 100, None) == -1 and b"null" in l.ccedit_last_error()
    assert l.ccedit_png_adler(16, 16, 16, 0, 100, None) == -1 and l.ccedit_png_adler(16, 16, 18, 1, 100, None) == -1


# ---- size ------------------------------------------------------------------------------------------
# The restatement's file over Pillow's default save(format="PNG") of the same pixels, measured + 0.02 for
# another zlib build behind Pillow.  The real frame is a 256 x 384 crop of the sample footage at its native resolution: smooth, so the
# deep chains and lazy matching of zlib level 6 (Pillow's default) find what a single-entry table cannot — zlib level 1 on the same
# filtered bytes reaches 1.169.
RATIOS = {"golden": 1.1710, "photo128": 0.9826, "photo512": 0.9812}


def _ratio(frame, tmp_path, name):
    path = M.write_apng(str(tmp_path / f"{name}.png"), frame[None], 50)
    assert (pillow_frames(path)[1][0] == frame).all()
    return os.path.getsize(path) / pillow_png_bytes(frame)


def test_size_against_pillow(tmp_path):
    from _gif_cases import content
    golden = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "png_bear_crop.png")).convert("RGB"))
    assert golden.shape == (256, 384, 3)
    got = {"golden": _ratio(golden, tmp_path, "golden"), "photo128": _ratio(np.ascontiguousarray(content("photo", 128, 192)), tmp_path, "p128"),
           "photo512": _ratio(np.ascontiguousarray(content("photo", 512, 768)), tmp_path, "p512")}
    print({k: round(v, 4) for k, v in got.items()})
    for k, v in got.items():
        assert v <= RATIOS[k] + 0.02, (k, v)


def test_size_conditions(tmp_path):
    """Two conditions, not measurements.  Noise: the file is at most the raw bytes + HEADER_MAX per chunk + the container.  Flat frames: the
    file is below 1 % of the raw H * W * 3 bytes, at the two sizes the ratios above are measured at (0.66 % and 0.33 %).  A frame of
    64 x 96 is too small for that figure to mean the coder: its file is 235 bytes = 1.27 %, of which 63 are the container, and a row of
    289 filtered bytes costs two matches because a match ends at 258 bytes."""
    noise = K.frame("noise", 64, 96)
    path = M.write_apng(str(tmp_path / "noise.png"), noise[None], 50)
    container = 8 + (12 + 13) + 12 + 12 + 2 + 4                           # signature, IHDR, IDAT and IEND framing, 78 01, Adler-32
    chunks = P.chunks_of(P.filtered_bytes(64, 96))
    assert os.path.getsize(path) <= P.filtered_bytes(64, 96) + chunks * P.HEADER_MAX + container
    assert P.HEADER_MAX == (P.HEADER_MAX_BITS + P.CHUNK // 256 + 9 + 7) // 8
    for h, w in ((128, 192), (512, 768)):
        flat = K.frame("flat", h, w)
        path = M.write_apng(str(tmp_path / f"flat{h}.png"), flat[None], 50)
        assert (pillow_frames(path)[1][0] == flat).all()
        assert os.path.getsize(path) < 0.01 * h * w * 3, os.path.getsize(path)
