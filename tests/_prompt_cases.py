"""A toy CLIP vocabulary for the prompt tests, in the format of the one tests/test_host_logic.py writes: the byte alphabet of byte-level
BPE, every byte again as a word end, two merges and the two special tokens — structurally a CLIP tokenizer, NOT the real one.  Every
lower-case letter that stands alone is ONE token (`a</w>`), a comma is one token (`,</w>`), `cat` is one token: prompts of an exact token
count are words of one letter."""
import json
import os


def write_toy_clip_tokenizer(d) -> dict:
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    chars, extra = [], 0
    for b in range(256):
        if b in keep:
            chars.append(chr(b))
        else:
            chars.append(chr(256 + extra))
            extra += 1
    vocab = {}
    for c in chars:
        vocab[c] = len(vocab)
    for c in chars:
        vocab[c + "</w>"] = len(vocab)
    merges = [("c", "a"), ("ca", "t</w>")]
    for a, b in merges:
        vocab[a + b] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    with open(os.path.join(str(d), "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(str(d), "merges.txt"), "w") as f:
        f.write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    return vocab


def toy_embedder(tmp_path, monkeypatch):
    """(FrozenCLIPEmbedder on the toy vocabulary, the vocabulary): `_expected_vocab` is swapped as test_host_logic.py swaps it."""
    from sgm.modules.encoders.modules import FrozenCLIPEmbedder
    vocab = write_toy_clip_tokenizer(tmp_path)
    monkeypatch.setattr(FrozenCLIPEmbedder, "_expected_vocab", None)
    return FrozenCLIPEmbedder(tokenizer_path=str(tmp_path)), vocab


def words(n: int, letter: str = "b") -> str:
    """A prompt of exactly n tokens of the toy vocabulary."""
    return " ".join([letter] * n)
