"""Long and weighted prompts without a GPU (ccedit_amd/prompt.py, --prompt_chunks / --prompt_syntax): the grammar and its refusals,
the chunk rule on a toy CLIP vocabulary (tests/_prompt_cases.py), the properties of the numpy restatement the kernel is held to
(tests/_prompt_numpy.py), the ids a conditioning file may carry, and the flags' defaults."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prompt_cases as PC  # noqa: E402
import _prompt_numpy as PN  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _args(*argv, ref=False):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return (R if ref else S).parse_args(list(argv))


# ---- 1. the grammar --------------------------------------------------------------------------------
def _parse(text, **kw):
    from ccedit_amd import prompt
    return prompt.parse(text, **kw)


def test_parser_weights():
    assert _parse("a cat") == [("a cat", 1.0)]
    assert _parse("(a)") == [("a", pytest.approx(1.1))]
    got = _parse("((a))")
    assert [t for t, _ in got] == ["a"] and got[0][1] == pytest.approx(1.21)
    assert _parse("[a]") == [("a", pytest.approx(1 / 1.1))]
    assert _parse("(a:0)") == [("a", 0.0)]
    assert _parse("(red coat:1.3) on a man") == [("red coat", 1.3), (" on a man", 1.0)]
    assert _parse("x (a (b:2) [[c]]) y") == [("x ", 1.0), ("a ", pytest.approx(1.1)), ("b", pytest.approx(2.2)), (" ", pytest.approx(1.1)),
                                             ("c", pytest.approx(1 / 1.1)), (" y", 1.0)]
    assert _parse("(a:8)") == [("a", 8.0)] and _parse("(a: 1.5 )") == [("a", 1.5)]
    # a colon that is followed by words is text, and a colon outside round brackets always is
    assert _parse("(a photo: night)") == [("a photo: night", pytest.approx(1.1))]
    assert _parse("ratio 4:3") == [("ratio 4:3", 1.0)]


def test_parser_escapes_and_plain_mode():
    assert _parse(r"\(a\) \[b\] \\") == [(r"(a) [b] " + "\\", 1.0)]
    assert _parse(r"(\(a\):2)") == [("(a)", 2.0)]
    assert _parse("(a:1.3) [b]", syntax="plain") == [("(a:1.3) [b]", 1.0)]              # brackets are text
    assert _parse("((a)", syntax="plain") == [("((a)", 1.0)]                            # ... and nothing is refused


def test_parser_break():
    from ccedit_amd.prompt import BREAK
    assert _parse("a BREAK b") == [("a ", 1.0), (BREAK, 1.0), (" b", 1.0)]
    assert _parse("a BREAK b", syntax="plain") == [("a ", 1.0), (BREAK, 1.0), (" b", 1.0)]
    assert _parse("a BREAK b", syntax="plain", breaks=False) == [("a BREAK b", 1.0)]
    assert _parse("BREAKFAST aBREAK BREAK") == [("BREAKFAST aBREAK ", 1.0), (BREAK, 1.0)]          # a whitespace-delimited WORD
    got = _parse("(a BREAK b:2)")                                                      # inside a group: the weight goes on after it
    assert [t for t, _ in got] == ["a ", BREAK, " b"] and got[0][1] == got[2][1] == 2.0


@pytest.mark.parametrize("text,pos,what", [
    ("a (b", 2, "unbalanced"), ("a b)", 3, "unbalanced"), ("(a]", 2, "unbalanced"), ("a [b", 2, "unbalanced"),
    ("(a:)", 2, "empty weight"), ("(a: )", 2, "empty weight"),
    ("xy (a:nan)", 5, "not finite"), ("(a:inf)", 2, "not finite"), ("(a:1e999)", 2, "not finite"),
    ("(a:8.5)", 2, "outside"), ("(a:-0.5)", 2, "outside"),
])
def test_parser_refusals_name_the_position(text, pos, what):
    with pytest.raises(ValueError, match=what) as e:
        _parse(text)
    assert f"position {pos}" in str(e.value), str(e.value)


# ---- 2. the chunk rule -----------------------------------------------------------------------------
@pytest.fixture()
def toy(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    return PC.toy_embedder(tmp_path, monkeypatch)


def _rows(enc, name):
    return enc[name]["tokens"][0].tolist(), enc[name]["weights"][0].tolist()


def test_75_tokens_are_one_chunk_and_76_are_two(toy):
    from ccedit_amd import prompt
    emb, vocab = toy
    tok = emb.tokenizer()
    bos, eos, b = vocab["<|startoftext|>"], vocab["<|endoftext|>"], vocab["b</w>"]
    assert prompt.comma_id(tok) == vocab[",</w>"]
    enc = prompt.encode_prompts(tok, {"p": PC.words(75)}, 4)
    assert enc["n"] == 1 and enc["p"]["prompt_tokens"] == 75 and enc["p"]["prompt_chunks"] == 1
    assert _rows(enc, "p")[0] == [bos] + [b] * 75 + [eos]
    enc = prompt.encode_prompts(tok, {"p": PC.words(76)}, 4)
    assert enc["n"] == 2 and enc["p"]["prompt_tokens"] == 76 and enc["p"]["tokens"].shape == (1, 154)
    assert _rows(enc, "p")[0] == [bos] + [b] * 75 + [eos] + [bos, b] + [eos] * 75
    assert _rows(enc, "p")[1] == [1.0] * 154
    enc = prompt.encode_prompts(tok, {"p": ""}, 4)                                       # an empty prompt is one chunk
    assert enc["n"] == 1 and _rows(enc, "p")[0] == [bos] + [eos] * 76 and enc["p"]["prompt_tokens"] == 0


@pytest.mark.parametrize("distance,first", [(20, 56), (21, 75), (1, 75)])
def test_comma_backtrack(toy, distance, first):
    """80 tokens with ONE comma as the token `distance` from the end of the full chunk (distance 1: its last token).  Within the last 20
    the chunk ends after the comma and what followed opens the next chunk; at 21 the cut is hard at 75."""
    from ccedit_amd import prompt
    emb, vocab = toy
    at = 75 - distance                                                                   # index of the comma among the 80 tokens
    text = " ".join(["b"] * at + [","] + ["b"] * (80 - at - 1))
    chunks, count = prompt.prompt_chunks(emb.tokenizer(), text)
    assert count == 80 and [len(c[0]) for c in chunks] == [first, 80 - first]
    if first < 75:
        assert chunks[0][0][-1] == vocab[",</w>"] and vocab[",</w>"] not in chunks[1][0]
    assert sum((c[0] for c in chunks), []) == [vocab["b</w>"]] * at + [vocab[",</w>"]] + [vocab["b</w>"]] * (80 - at - 1)      # nothing lost


def test_break_ends_a_chunk_and_weights_follow_their_tokens(toy):
    from ccedit_amd import prompt
    emb, vocab = toy
    tok = emb.tokenizer()
    bos, eos, a, b = vocab["<|startoftext|>"], vocab["<|endoftext|>"], vocab["a</w>"], vocab["b</w>"]
    enc = prompt.encode_prompts(tok, {"p": "a (b:1.5) BREAK [b] a"}, 2, "weighted")
    ids, ws = _rows(enc, "p")
    assert enc["n"] == 2 and enc["p"]["prompt_tokens"] == 4
    assert ids == [bos, a, b] + [eos] * 74 + [bos, b, a] + [eos] * 74
    assert ws[:3] == [1.0, 1.0, 1.5] and ws[3:77] == [1.0] * 74                          # BOS, EOS and padding weigh 1
    assert ws[77:80] == [1.0, pytest.approx(1 / 1.1), 1.0] and ws[80:] == [1.0] * 74
    # plain with one chunk does not look for BREAK (and here the word has no token: the toy vocabulary spells it in letters)
    assert prompt.encode_prompts(tok, {"p": "a BREAK b"}, 2)["n"] == 2
    assert prompt.encode_prompts(tok, {"p": "a BREAK b"}, 1)["n"] == 1


def test_the_shorter_prompts_are_padded_with_empty_chunks(toy):
    from ccedit_amd import prompt
    emb, vocab = toy
    bos, eos, b = vocab["<|startoftext|>"], vocab["<|endoftext|>"], vocab["b</w>"]
    enc = prompt.encode_prompts(emb.tokenizer(), {"--prompt": PC.words(160), "--negative_prompt": "b b", "--region_prompt 1": PC.words(80)}, 3)
    assert enc["n"] == 3
    assert [enc[k]["prompt_chunks"] for k in ("--prompt", "--negative_prompt", "--region_prompt 1")] == [3, 1, 2]
    assert all(enc[k]["tokens"].shape == (1, 231) and enc[k]["weights"].shape == (1, 231) for k in ("--prompt", "--negative_prompt", "--region_prompt 1"))
    neg = _rows(enc, "--negative_prompt")[0]
    assert neg == [bos, b, b] + [eos] * 74 + ([bos] + [eos] * 76) * 2
    assert _rows(enc, "--region_prompt 1")[0][154:] == [bos] + [eos] * 76


def test_a_prompt_above_prompt_chunks_is_refused_not_truncated(toy):
    from ccedit_amd import prompt
    emb, _ = toy
    with pytest.raises(ValueError, match=r"--negative_prompt: 160 tokens need 3 chunks .* --prompt_chunks is 2"):
        prompt.encode_prompts(emb.tokenizer(), {"--prompt": "b", "--negative_prompt": PC.words(160)}, 2)
    with pytest.raises(ValueError, match=r"--prompt: 76 tokens need 2 chunks"):
        prompt.encode_prompts(emb.tokenizer(), {"--prompt": PC.words(76)}, 1, "weighted")
    with pytest.raises(ValueError, match=r"--prompt: prompt: unbalanced '\(' at position 2"):
        prompt.encode_prompts(emb.tokenizer(), {"--prompt": "b (b"}, 2, "weighted")
    with pytest.raises(ValueError, match="prompt_chunks 5"):
        prompt.encode_prompts(emb.tokenizer(), {"--prompt": "b"}, 5)


@pytest.mark.parametrize("text", ["a cat", "masterpiece, high quality, a cat", "", PC.words(75), "A Cat,  and (a) [dog]"])
def test_a_short_plain_prompt_gives_the_ids_of_tokenize(toy, text):
    from ccedit_amd import prompt
    emb, _ = toy
    want = emb.tokenize([text])
    for chunks in (1, 4):
        enc = prompt.encode_prompts(emb.tokenizer(), {"p": text}, chunks)
        assert torch.equal(enc["p"]["tokens"], want), (text, chunks)
    if "(" not in text:
        assert torch.equal(prompt.encode_prompts(emb.tokenizer(), {"p": text}, 1, "weighted")["p"]["tokens"], want)


# ---- 3. the restatement, and ids from outside ----------------------------------------------------------
def _zew(b, n, c, seed):
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((b, 77 * n, c)).astype(np.float32)
    e = rs.standard_normal((77, c)).astype(np.float32)
    w = rs.choice(np.array([0, 0.5, 1, 1.1, 1.21, 8], np.float32), size=(b, 77 * n))
    return z, e, w


def test_restatement_weight_one_is_z_and_weight_zero_is_e():
    z, e, w = _zew(2, 3, 8, 0)
    z[0, 0, 0], z[0, 1, 1], z[1, 5, 2] = 1e30, -1e-30, np.float32(np.nan)
    one = PN.prompt_weight(z, e, np.ones_like(w))
    assert np.array_equal(one.view(np.int32), z.view(np.int32))                          # the bits, NaN payload included
    zero = PN.prompt_weight(z, e, np.zeros_like(w))
    fin = np.isfinite(z)
    assert np.array_equal(zero[fin], np.broadcast_to(np.tile(e, (3, 1))[None], z.shape)[fin])
    # e + (z - e) is NOT z in floating point: the branch is needed
    naive = (np.tile(e, (3, 1))[None] + (z - np.tile(e, (3, 1))[None])).astype(np.float32)
    assert not np.array_equal(naive[fin], z[fin])
    mixed = PN.prompt_weight(z, e, w)
    rows = w == 1
    assert rows.any() and (~rows).any() and np.array_equal(mixed[rows].view(np.int32), z[rows].view(np.int32))
    half = PN.prompt_weight(z, e, np.full_like(w, 0.5))
    et = np.tile(e, (3, 1))[None]
    assert np.array_equal(half[fin], (et + np.float32(0.5) * (z - et))[fin])


def test_ids_of_whole_chunks_are_accepted_and_others_refused():
    from ccedit_amd import prompt
    for n in (1, 2, 3, 4):
        ids = torch.zeros((1, 77 * n), dtype=torch.int64)
        assert prompt.check_tokens(ids) == n
        assert prompt.check_tokens(ids, torch.ones((1, 77 * n))) == n
    for bad in (77 * 2 + 1, 76, 77 * 5, 0):
        with pytest.raises(ValueError, match="chunks of 77"):
            prompt.check_tokens(torch.zeros((1, bad), dtype=torch.int64))
    ids = torch.zeros((1, 154), dtype=torch.int64)
    with pytest.raises(ValueError, match="shape"):
        prompt.check_tokens(ids, torch.ones((1, 77)))
    for v in (float("nan"), float("inf"), -1.0, 8.5):
        w = torch.ones((1, 154))
        w[0, 3] = v
        with pytest.raises(ValueError, match="not finite or outside"):
            prompt.check_tokens(ids, w)
    t, w = prompt.pad_tokens(torch.full((2, 77), 5), torch.full((2, 77), 0.5), 3, 1, 2)
    assert t.shape == (2, 231) and t[1, 77:].tolist() == ([1] + [2] * 76) * 2 and w[0].tolist() == [0.5] * 77 + [1.0] * 154


def test_cond_file_ids_reach_the_new_path_only_when_they_ask_for_it():
    """cond_text: None (the path as before) for (1, 77) ids with default flags; longer ids or weights go through encode_long, the two
    halves padded to one length; 77 n + 1 ids are refused before the embedder is touched."""
    from scripts.sampling import sampling_tv2v as S

    class Emb:
        input_key = "txt"

        def special_ids(self):
            return 1, 2

        def encode_long(self, tokens, weights=None):
            self.calls.append((tokens.clone(), None if weights is None else weights.clone()))
            return torch.zeros(tokens.shape + (4,))

    class Model:
        pass
    emb, model = Emb(), Model()
    emb.calls = []
    model.conditioner = Model()
    model.conditioner.embedders = [emb]
    ids = lambda l: torch.full((1, l), 7, dtype=torch.int64)
    assert S.cond_text(_args(), model, dict(tokens=ids(77), tokens_uc=ids(77)), "cpu") is None and not emb.calls
    assert S.cond_text(_args(), model, dict(crossattn=torch.zeros(1, 77, 4), crossattn_uc=torch.zeros(1, 77, 4)), "cpu") is None
    txt, txt_uc, log = S.cond_text(_args(), model, dict(tokens=ids(231), tokens_uc=ids(77)), "cpu")
    assert txt.shape == (1, 231, 4) and txt_uc.shape == (1, 231, 4)
    assert emb.calls[1][0][0, 77:].tolist() == ([1] + [2] * 76) * 2 and emb.calls[0][1] is None
    assert log == [dict(prompt_tokens=None, prompt_chunks=3, negative_prompt_tokens=None, negative_prompt_chunks=1, context_rows=231)]
    emb.calls.clear()
    S.cond_text(_args(), model, dict(tokens=ids(77), tokens_uc=ids(77), token_weights=torch.full((1, 77), 0.5)), "cpu")
    assert emb.calls[0][1].tolist() == [[0.5] * 77] and emb.calls[1][1].tolist() == [[1.0] * 77]
    emb.calls.clear()
    with pytest.raises(ValueError, match="chunks of 77"):
        S.cond_text(_args(), model, dict(tokens=ids(155), tokens_uc=ids(77)), "cpu")
    assert not emb.calls


# ---- 4. the flags ------------------------------------------------------------------------------------
def test_flag_defaults_leave_the_text_path_alone(toy):
    from scripts.sampling import sampling_tv2v as S
    emb, _ = toy
    for ref in (False, True):
        a = _args(ref=ref)
        assert (a.prompt_chunks, a.prompt_syntax) == (1, "plain") and not S.prompts_on(a)
    a = _args("--prompt", "a (cat)", "--tokenizer_path", emb.tokenizer_path)
    assert S.text_inputs({}, "cpu", a) == (["masterpiece, high quality, a (cat)"], ["ugly, low quality"])
    cond = dict(tokens=torch.arange(77)[None], tokens_uc=torch.arange(77)[None] + 1)
    txt, txt_uc = S.text_inputs(cond, "cpu", _args())
    assert torch.equal(txt, cond["tokens"]) and torch.equal(txt_uc, cond["tokens_uc"])
    assert S.job_text(a, ["a (cat)"], "cpu", 768) == (["masterpiece, high quality, a (cat)"], ["ugly, low quality"])
    assert S.prompts_on(_args("--prompt_chunks", "2")) and S.prompts_on(_args("--prompt_syntax", "weighted"))
    assert S.prompts_on(_args("--prompt_chunks", "4", ref=True))
    for bad in (["--prompt_chunks", "0"], ["--prompt_chunks", "5"], ["--prompt_syntax", "loud"]):
        with pytest.raises(SystemExit):
            _args(*bad)


def test_synthetic_ids_follow_prompt_chunks():
    from scripts.sampling import sampling_tv2v as S
    a = _args("--synthetic", "--num_keyframes", "1", "--H", "8", "--W", "8")
    a.context_dim = 768
    one = S.conditioning_tensors(a, torch.Generator().manual_seed(3), False)
    a3 = _args("--synthetic", "--num_keyframes", "1", "--H", "8", "--W", "8", "--prompt_chunks", "3")
    a3.context_dim = 768
    three = S.conditioning_tensors(a3, torch.Generator().manual_seed(3), False)
    assert one["tokens"].shape == (1, 77) and three["tokens"].shape == (1, 231) and three["tokens_uc"].shape == (1, 231)
    assert torch.equal(one["tokens"], torch.randint(0, 49406, (1, 77), generator=torch.Generator().manual_seed(3)))      # as before


def test_a_truncated_prompt_is_announced_on_the_old_path(toy, capsys):
    from scripts.sampling import sampling_tv2v as S
    emb, _ = toy

    class Model:
        pass
    model = Model()
    model.conditioner = Model()
    model.conditioner.embedders = [emb]
    emb.input_key = "txt"
    a = _args("--tokenizer_path", emb.tokenizer_path)
    S.warn_truncated(a, model, [PC.words(75), PC.words(100)])
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 1 and err[0].startswith("[prompt] 100 tokens") and "--prompt_chunks 2" in err[0]
    S.warn_truncated(_args("--tokenizer_path", emb.tokenizer_path, "--prompt_chunks", "2"), model, [PC.words(100)])
    assert capsys.readouterr().err == ""


def test_the_entry_point_is_declared_bound_and_built():
    from ccedit_amd import hip
    from ccedit_amd.csrc import build
    assert "ccedit_prompt_weight" in hip.EXPORTS
    assert "prompt.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["prompt.hip"]
    lib = hip.lib()
    assert lib.ccedit_prompt_weight(None, None, None, None, 1, 77, 768, None) == -1 and b"null pointer" in lib.ccedit_last_error()
    assert lib.ccedit_prompt_weight(16, 16, 16, 16, 1, 78, 768, None) == -1 and b"multiple of 77" in lib.ccedit_last_error()
