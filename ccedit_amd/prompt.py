"""Long and weighted prompts: the host side.

The CLIP text encoder sees 77 tokens, 75 of them the prompt's; the reference truncates what is beyond (encoders/modules.py:396-404).
With `--prompt_chunks N` (N <= 4) a prompt is cut into up to N chunks of 75 tokens, every chunk is encoded on its own as
`[BOS] + tokens + [EOS]` padded with EOS to 77, and the encodings are laid side by side: a context of L = 77 n rows, which the network's
text cross-attention takes like any other.  With `--prompt_syntax weighted` the prompt may carry emphasis — `(x)`, `[x]`, `(x:1.3)` — and
every token carries a weight, applied to the encoder's OUTPUT by `ccedit_prompt_weight` (csrc/prompt.hip).

Everything here is host code on Python lists: `parse` (the grammar), `chunk_tokens` (the chunk rule), `encode_prompts` (the prompts of
one clip to id and weight rows of ONE length) and the checks of ids that come from a conditioning file.  Nothing touches the GPU, and
every refusal is a ValueError raised before any GPU work.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

CHUNK = 77                   # tokens the text encoder sees
BODY = CHUNK - 2             # ... of which the prompt's: BOS and one EOS are the encoder's
MAX_CHUNKS = 4               # --prompt_chunks 1 ... 4: a context of at most 308 rows
BACKTRACK = 20               # a chunk that is full ends after the last comma among its last 20 tokens, if there is one
UP = 1.1                     # (x) multiplies by UP, [x] divides by it
W_MAX = 8.0                  # an explicit weight lies in [0, W_MAX]
SYNTAXES = ("plain", "weighted")
BREAK = None                 # the piece of parse()'s list that ends the current chunk

Piece = Tuple[Optional[str], float]


def check_options(chunks: int, syntax: str) -> None:
    if not 1 <= int(chunks) <= MAX_CHUNKS:
        raise ValueError(f"--prompt_chunks {chunks}: a prompt may use 1 ... {MAX_CHUNKS} chunks of {CHUNK} tokens")
    if syntax not in SYNTAXES:
        raise ValueError(f"--prompt_syntax {syntax!r}: one of {', '.join(SYNTAXES)}")


# ------------------------------------------------------------------------------------------
# Grammar
# ------------------------------------------------------------------------------------------
def _is_break(text: str, i: int) -> bool:
    """The whitespace-delimited word BREAK at text[i:]."""
    return (text.startswith("BREAK", i) and (i == 0 or text[i - 1].isspace()) and (i + 5 == len(text) or text[i + 5].isspace()))


def _weight(s: str, pos: int) -> float:
    """The number after the colon of `(x:NUMBER)`; `pos` is the colon's position."""
    try:
        v = float(s)
    except ValueError:
        raise ValueError(f"prompt: weight {s!r} after ':' at position {pos} is not a number") from None
    if not math.isfinite(v):
        raise ValueError(f"prompt: weight {s!r} after ':' at position {pos} is not finite")
    if not 0.0 <= v <= W_MAX:
        raise ValueError(f"prompt: weight {s!r} after ':' at position {pos} is outside [0, {W_MAX:g}]")
    return v


def _looks_numeric(s: str) -> bool:
    """What follows a colon is meant as a weight when it is empty or starts like a number (`nan`, `inf` included: they are refused, not
    read as text); anything else — `(a photo: night)` — leaves the colon a literal and the group an ordinary `(x)`."""
    t = s.lstrip("+-").lower()
    return s == "" or t[:1].isdigit() or t[:1] == "." or t.startswith(("nan", "inf"))


def parse(text: str, syntax: str = "weighted", breaks: bool = True) -> List[Piece]:
    """The prompt as [(text piece, weight)]; a `(BREAK, 1.0)` entry (BREAK is None) where the word BREAK ends the current chunk.
    plain: one piece of weight 1, cut only at BREAK (if `breaks`).  weighted: `(x)` multiplies the weight of x by 1.1, `[x]` divides
    it by 1.1, `(x:1.3)` multiplies it by the given factor instead, nesting multiplies; `\\(`, `\\)`, `\\[`, `\\]`, `\\\\` are literals.
    Neighbouring pieces of equal weight are joined.  ValueError, with the character position counted from 0: an unbalanced bracket,
    an empty weight, a weight that is not finite or outside [0, 8]."""
    if syntax not in SYNTAXES:
        raise ValueError(f"prompt syntax {syntax!r}: one of {', '.join(SYNTAXES)}")
    weighted = syntax == "weighted"
    pieces: List[list] = []              # [text or BREAK, weight]
    stack: List[list] = []               # [bracket, position, first piece of the group, index of the last colon's piece or -1, colon position]
    buf: List[str] = []

    def flush():
        if buf:
            pieces.append(["".join(buf), 1.0])
            buf.clear()

    i, n = 0, len(text)
    while i < n:
        ch = text[i]
        if breaks and ch == "B" and _is_break(text, i):
            flush()
            pieces.append([BREAK, 1.0])
            i += 5
            continue
        if not weighted:
            buf.append(ch)
        elif ch == "\\" and i + 1 < n and text[i + 1] in "()[]\\":
            buf.append(text[i + 1])
            i += 1
        elif ch in "([":
            flush()
            stack.append([ch, i, len(pieces), -1, -1])
        elif ch == ":" and stack and stack[-1][0] == "(":
            flush()
            stack[-1][3], stack[-1][4] = len(pieces), i          # the LAST colon of the group counts; an earlier one stays text
            pieces.append([":", 1.0])
        elif ch in ")]":
            flush()
            if not stack or stack[-1][0] != ("(" if ch == ")" else "["):
                raise ValueError(f"prompt: unbalanced {ch!r} at position {i}" + (f" (the {stack[-1][0]!r} at position {stack[-1][1]} is still open)"
                                                                                 if stack else " (nothing is open)"))
            _, _, first, colon, cpos = stack.pop()
            factor = UP if ch == ")" else 1.0 / UP
            if colon >= 0 and all(p[0] is not BREAK and p[1] == 1.0 for p in pieces[colon + 1:]):
                tail = "".join(p[0] for p in pieces[colon + 1:]).strip()
                if _looks_numeric(tail):
                    if tail == "":
                        raise ValueError(f"prompt: empty weight after ':' at position {cpos}")
                    factor = _weight(tail, cpos)
                    del pieces[colon:]
            for p in pieces[first:]:                              # (an outer group's colon lies before `first`: its index still holds)
                p[1] *= factor
        else:
            buf.append(ch)
        i += 1
    flush()
    if stack:
        raise ValueError(f"prompt: unbalanced {stack[-1][0]!r} at position {stack[-1][1]} (never closed)")
    out: List[Piece] = []
    for t, w in pieces:
        if t is not BREAK and out and out[-1][0] is not BREAK and out[-1][1] == w:
            out[-1] = (out[-1][0] + t, w)
        elif t is BREAK or t != "":
            out.append((t, float(w)))
    return out


# ------------------------------------------------------------------------------------------
# Tokens and chunks
# ------------------------------------------------------------------------------------------
def comma_id(tok) -> Optional[int]:
    """The id of the tokenizer's comma token (looked up, never assumed: toy vocabularies work), or None when a comma is not one token."""
    ids = tok(",", add_special_tokens=False)["input_ids"]
    return int(ids[0]) if len(ids) == 1 else None


def tokenize_pieces(tok, pieces: Sequence[Piece]) -> List[Tuple[List[int], List[float]]]:
    """Every piece is tokenised on its own (no special tokens) and every token inherits its piece's weight.  Returns the segments
    between BREAKs as (ids, weights); there is always at least one segment."""
    segs: List[Tuple[List[int], List[float]]] = [([], [])]
    for t, w in pieces:
        if t is BREAK:
            segs.append(([], []))
            continue
        ids = [int(v) for v in tok(t, add_special_tokens=False)["input_ids"]]
        segs[-1][0].extend(ids)
        segs[-1][1].extend([float(w)] * len(ids))
    return segs


def chunk_tokens(ids: Sequence[int], weights: Sequence[float], comma: Optional[int]) -> List[Tuple[List[int], List[float]]]:
    """One segment -> chunks of at most 75 tokens.  When the next token does not fit and the chunk's last 20 tokens contain the comma
    token, the chunk ends after the LAST such comma and what followed it opens the next chunk; otherwise the cut is hard at 75.
    An empty segment is one empty chunk."""
    chunks: List[Tuple[List[int], List[float]]] = []
    ci: List[int] = []
    cw: List[float] = []
    for t, w in zip(ids, weights):
        if len(ci) == BODY:
            cut = BODY
            if comma is not None:
                for j in range(BODY - 1, BODY - BACKTRACK - 1, -1):
                    if ci[j] == comma:
                        cut = j + 1
                        break
            chunks.append((ci[:cut], cw[:cut]))
            ci, cw = ci[cut:], cw[cut:]
        ci.append(int(t))
        cw.append(float(w))
    chunks.append((ci, cw))
    return chunks


def prompt_chunks(tok, text: str, syntax: str = "plain", breaks: bool = True) -> Tuple[List[Tuple[List[int], List[float]]], int]:
    """A prompt -> (its chunks as (ids, weights) of at most 75 tokens, its token count)."""
    comma = comma_id(tok)
    chunks: List[Tuple[List[int], List[float]]] = []
    count = 0
    for ids, ws in tokenize_pieces(tok, parse(text, syntax, breaks)):
        count += len(ids)
        chunks += chunk_tokens(ids, ws, comma)
    return chunks, count


def assemble(chunks, n: int, bos: int, eos: int) -> Tuple[List[int], List[float]]:
    """Chunks -> one row of 77 n ids and one of weights: every chunk `[BOS] + tokens + [EOS]` padded with EOS to 77, then empty chunks
    (BOS, EOS x 76) up to n.  BOS, EOS and padding have weight 1."""
    ids: List[int] = []
    ws: List[float] = []
    for k in range(n):
        ci, cw = chunks[k] if k < len(chunks) else ([], [])
        assert len(ci) <= BODY
        ids += [bos] + list(ci) + [eos] * (CHUNK - 1 - len(ci))
        ws += [1.0] + list(cw) + [1.0] * (CHUNK - 1 - len(cw))
    return ids, ws


def encode_prompts(tok, prompts: Dict[str, str], max_chunks: int = 1, syntax: str = "plain") -> dict:
    """The prompts of one clip — {name: text}, e.g. prompt, negative_prompt, region_prompt 1 ... — to rows of ONE length: n is the largest
    chunk count among them and the others are padded with empty chunks, because the halves of classifier-free guidance are
    concatenated and the regions share one graph shape.  Returns {name: dict(tokens int64 (1, 77 n), weights fp32 (1, 77 n),
    prompt_tokens, prompt_chunks)} and, under "n", n.  A prompt that needs more than `max_chunks` chunks is a ValueError that names it,
    its token count and the chunks it needs: nothing is ever truncated here."""
    check_options(max_chunks, syntax)
    bos, eos = int(tok.bos_token_id), int(tok.eos_token_id)
    breaks = max_chunks > 1 or syntax == "weighted"
    cut = {}
    for name, text in prompts.items():
        try:
            chunks, count = prompt_chunks(tok, text, syntax, breaks)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if len(chunks) > max_chunks:
            raise ValueError(f"{name}: {count} tokens need {len(chunks)} chunks of {BODY} but --prompt_chunks is {max_chunks} — raise "
                             f"--prompt_chunks (up to {MAX_CHUNKS}) or shorten the prompt; nothing is truncated")
        cut[name] = (chunks, count)
    n = max(len(c) for c, _ in cut.values())
    out: dict = {"n": n}
    for name, (chunks, count) in cut.items():
        ids, ws = assemble(chunks, n, bos, eos)
        out[name] = dict(tokens=torch.tensor([ids], dtype=torch.int64), weights=torch.tensor([ws], dtype=torch.float32),
                         prompt_tokens=count, prompt_chunks=len(chunks))
    return out


# ------------------------------------------------------------------------------------------
# Ids that come from outside (a conditioning file, a caller of the library)
# ------------------------------------------------------------------------------------------
def check_tokens(tokens: torch.Tensor, weights: Optional[torch.Tensor] = None, name: str = "tokens") -> int:
    """`tokens` must be integer (B, 77 n) with 1 <= n <= 4 and `weights`, if given, finite floats of the same shape in [0, 8].
    Returns n."""
    if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.is_floating_point():
        raise ValueError(f"{name}: expected integer token ids (B, {CHUNK} n), got "
                         f"{tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__}")
    l = int(tokens.shape[1])
    if l == 0 or l % CHUNK or l // CHUNK > MAX_CHUNKS:
        raise ValueError(f"{name}: {l} ids per row — whole chunks of {CHUNK} are expected, 1 ... {MAX_CHUNKS} of them "
                         f"({', '.join(str(CHUNK * k) for k in range(1, MAX_CHUNKS + 1))})")
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) != tuple(tokens.shape) or not weights.is_floating_point():
            raise ValueError(f"{name}: the weights must be floats of the ids' shape {tuple(tokens.shape)}, got "
                             f"{tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__}")
        if not bool(torch.isfinite(weights).all()) or float(weights.min()) < 0.0 or float(weights.max()) > W_MAX:
            raise ValueError(f"{name}: a weight is not finite or outside [0, {W_MAX:g}]")
    return l // CHUNK


def pad_tokens(tokens: torch.Tensor, weights: Optional[torch.Tensor], n: int, bos: int, eos: int):
    """(B, 77 m) ids (and weights) -> (B, 77 n), m <= n, by appending empty chunks (BOS, EOS x 76; weight 1)."""
    b, l = tokens.shape
    m = l // CHUNK
    if m == n:
        return tokens, weights
    empty = torch.tensor([[bos] + [eos] * (CHUNK - 1)], dtype=tokens.dtype, device=tokens.device).repeat(b, n - m)
    tokens = torch.cat([tokens, empty], dim=1)
    if weights is not None:
        weights = torch.cat([weights, torch.ones((b, CHUNK * (n - m)), dtype=weights.dtype, device=weights.device)], dim=1)
    return tokens, weights
