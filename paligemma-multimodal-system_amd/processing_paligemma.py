"""Image/prompt pre-processing — drop-in for the reference's ``processing_paligemma`` (host side).

Behaviour of processing_paligemma.py:13-212: PIL bicubic resize to (image_size, image_size),
RGB, x/255 in fp32, (x - 0.5)/0.5, HWC -> CHW, batch stack; the "gemma string"
``<image>*N + <bos> + prompt + "\\n"`` tokenised with the image token and 128 <seg> / 1024
<loc> tokens added to the tokenizer.  As in the reference, ``__call__`` passes the LIST of
prompts to the string builder, so the prompt text is the list's repr (e.g. ``['caption en']``,
SURVEY.md §8(c)) — kept for output parity.  Batch size 1, as the reference asserts.
Host-only code (PIL / numpy / tokenizer); the image tensor it returns is what the HIP path consumes.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

IMAGENET_STANDARD_MEAN = [0.5, 0.5, 0.5]
IMAGENET_STANDARD_STD = [0.5, 0.5, 0.5]


def resize(image, resampling, image_size: int, reducing_gap: Optional[int] = None):
    return image.resize((image_size, image_size), resample=resampling, reducing_gap=reducing_gap)


def rescale(image: np.ndarray, scale_factor: float, dtype=np.float32) -> np.ndarray:
    return (image * scale_factor).astype(dtype)


def normalise(image: np.ndarray, mean: Union[float, Sequence[float]], std: Union[float, Sequence[float]]):
    return (image - np.asarray(mean, dtype=image.dtype)) / np.asarray(std, dtype=image.dtype)


def process_images(images: List, image_size: int, scale_factor: float, resampling=None,
                   reducing_gap: Optional[int] = None) -> List[np.ndarray]:
    """resize -> RGB -> rescale -> normalise -> CHW, per image (processing_paligemma.py:38-73)."""
    out = []
    for im in images:
        arr = np.array(resize(im, resampling, image_size, reducing_gap).convert("RGB"))
        arr = normalise(rescale(arr, scale_factor), IMAGENET_STANDARD_MEAN, IMAGENET_STANDARD_STD)
        out.append(arr.transpose(2, 0, 1))
    return out


def create_gemma_string(prefix_prompt, image_seq_len: int, image_token: str, bos_token: str) -> str:
    """<image>*N <bos> prompt \\n (processing_paligemma.py:77-89)."""
    return f"{image_token * image_seq_len}{bos_token}{prefix_prompt}\n"


class PaliGemmaProcessor:
    """Tokenizer + image pipeline (processing_paligemma.py:94-212)."""

    IMAGE_TOKEN = "<image>"

    def __init__(self, tokenizer, num_image_tokens: int, image_size: int, device=None):
        """device: when a HIP device is given, images of the modes in pghip.image.SUPPORTED_MODES (RGB, RGBA, LA,
        L, P, 1) are resized/normalised there (bit-exact with the host path below) and any other mode (CMYK, I, F, ...)
        takes the host path; None keeps the reference's host (PIL + numpy) path for every image."""
        self.device = device
        self.tokenizer = tokenizer
        self.image_seq_len = num_image_tokens
        self.image_size = image_size
        tokenizer.add_special_tokens({"additional_special_tokens": [self.IMAGE_TOKEN]})
        extra = [f"<seg{i:03d}>" for i in range(128)] + [f"<loc{i:04d}>" for i in range(1024)]
        tokenizer.add_tokens(extra)
        tokenizer.image_token_id = tokenizer.convert_tokens_to_ids(self.IMAGE_TOKEN)
        tokenizer.add_eos_token = False
        tokenizer.add_bos_token = False

    def __call__(self, images: List, text: List[str], padding: str = "longest", truncation: bool = True):
        assert len(images) == 1 and len(text) == 1, \
            "Working with only 1 image and prompt, to test, got more than one"
        from PIL import Image
        gpu_image = None
        if self.device is not None:
            from pghip import image as gpu_image
        if gpu_image is not None and all(getattr(im, "mode", None) in gpu_image.SUPPORTED_MODES for im in images):
            pixel_values = gpu_image.preprocess(images, self.image_size, self.device)
        else:
            pixel_values = torch.tensor(np.stack(process_images(images, self.image_size, scale_factor=1 / 255.0,
                                                                resampling=Image.Resampling.BICUBIC), axis=0))
        s = create_gemma_string(prefix_prompt=text, image_seq_len=self.image_seq_len, image_token=self.IMAGE_TOKEN,
                                bos_token=self.tokenizer.bos_token)
        toks = self.tokenizer(s, return_tensors="pt", truncation=truncation, padding=padding)
        return {"pixel_values": pixel_values, **toks}

    # ------------------------------------------------------------------ constrained decoding (pghip/grammar.py)
    def _ids(self, text: str, known: bool = False) -> List[int]:
        ids = list(self.tokenizer(text, add_special_tokens=False)["input_ids"])
        unk = getattr(self.tokenizer, "unk_token_id", None)
        if known and unk is not None and unk in ids:
            raise ValueError(f"{text!r} holds a word the tokenizer does not know (<unk>): it cannot be generated")
        return ids

    def detect_grammar(self, labels: Sequence[str], vocab: Optional[int] = None):
        """The TokenDFA of a ``detect a ; b`` answer: ``<loc><loc><loc><loc> label`` boxes separated by `` ;``, then
        ``<eos>``, or ``<eos>`` alone (TokenDFA.detect).  Pass it to ``generate(..., grammar=...)``; parse_detections
        reads the result.  vocab: the model's vocabulary size (config.vocab_size) when it exceeds the tokenizer's
        length, which is the default; ids past the tokenizer are never allowed.

        Limitation: a label is accepted only in the tokenisation the tokenizer gives for ``" " + label``
        (add_special_tokens=False), not in every token sequence that decodes to the same text."""
        from pghip.grammar import TokenDFA
        labels = [str(lb).strip() for lb in labels]
        if not labels or any(not lb for lb in labels):
            raise ValueError(f"detect_grammar: needs non-empty labels, got {labels!r}")
        tok = self.tokenizer
        loc_ids = tok.convert_tokens_to_ids([f"<loc{i:04d}>" for i in range(1024)])
        if tok.eos_token_id is None or any(i is None or i == tok.unk_token_id for i in loc_ids):
            raise ValueError("detect_grammar: the tokenizer lacks <eos> or the <loc> tokens")
        vocab = len(tok) if vocab is None else int(vocab)
        # (a model whose vocabulary stops inside the <loc> range can only ever emit the ids below it)
        dfa = TokenDFA.detect([i for i in loc_ids if i < vocab], [self._ids(" " + lb, True) for lb in labels],
                              self._ids(" ;"), tok.eos_token_id, vocab)
        dfa.meta.update(labels=labels, loc_ids=loc_ids)         # loc_ids[n] is <locNNNN>, for parse_detections
        self._detect_dfa = dfa
        return dfa

    def choices_grammar(self, choices: Sequence[str], vocab: Optional[int] = None):
        """The TokenDFA of a closed answer set: one of `choices`, tokenised as the tokenizer gives them, then ``<eos>``
        (TokenDFA.from_choices; vocab as detect_grammar; the same tokenisation limitation)."""
        from pghip.grammar import TokenDFA
        choices = [str(c) for c in choices]
        if not choices or any(not c.strip() for c in choices):
            raise ValueError(f"choices_grammar: needs non-empty choices, got {choices!r}")
        tok = self.tokenizer
        if tok.eos_token_id is None:
            raise ValueError("choices_grammar: the tokenizer has no <eos>")
        dfa = TokenDFA.from_choices([self._ids(c, True) for c in choices], tok.eos_token_id,
                                    len(tok) if vocab is None else int(vocab))
        dfa.meta["choices"] = choices
        return dfa

    def parse_detections(self, ids_or_text, height: int, width: int, grammar=None) -> List[dict]:
        """A constrained ``detect`` answer as ``[{"label": str, "box": (y_min, x_min, y_max, x_max)}]`` in pixels of a
        height x width image: ``<locNNNN>`` is NNNN / 1024 of the height (a box's first and third) or of the width
        (second and fourth).  ids_or_text: the generated ids, ending at ``<eos>`` (a tensor, or a list), or the decoded
        text (tokenised again; its ``<eos>`` may be missing).  grammar: the detect grammar the answer was generated
        under, by default the last one detect_grammar built.  A sequence that grammar does not accept (TokenDFA.accepts)
        raises ValueError naming the position of the first token it refuses."""
        dfa = grammar if grammar is not None else getattr(self, "_detect_dfa", None)
        if dfa is None or dfa.meta.get("kind") != "detect":
            raise ValueError("parse_detections: needs a detect grammar (call detect_grammar first, or pass grammar=)")
        m = dfa.meta
        if isinstance(ids_or_text, str):
            ids = self._ids(ids_or_text)
            if not ids or ids[-1] != m["eos"]:
                ids.append(m["eos"])
        else:
            ids = [int(t) for t in (ids_or_text.reshape(-1).tolist() if hasattr(ids_or_text, "reshape")
                                    else ids_or_text)]
        if not dfa.accepts(ids):
            _, n = dfa.walk(ids)
            what = f"token {ids[n]} at position {n}" if n < len(ids) else f"its end at position {n} (no <eos>)"
            raise ValueError(f"parse_detections: not a detect answer for labels {m.get('labels')}: {what} is not "
                             "allowed by the grammar")
        loc = {t: i for i, t in enumerate(m["loc_ids"])}
        names = {tuple(q): lb for q, lb in zip(m.get("label_seqs", ()), m.get("labels", ()))}
        out, s, coords, label_from = [], dfa.start, [], None

        def close(upto: int):
            y0, x0, y1, x1 = coords
            text = names.get(tuple(ids[label_from:upto]))       # the label as it was given, not a re-decoded spelling
            if text is None:
                text = self.tokenizer.decode(ids[label_from:upto], skip_special_tokens=True).strip()
            out.append({"label": text, "box": (y0 / 1024 * height, x0 / 1024 * width, y1 / 1024 * height,
                                               x1 / 1024 * width)})

        for i, t in enumerate(ids):
            s = dfa.step(s, t)
            if t in loc and label_from is None:
                coords.append(loc[t])
            if s == m["label_state"]:
                label_from = i + 1
            elif label_from is not None and (s == m["box_state"] or s in dfa.final):
                close(i + 1 - (m["sep_len"] if s == m["box_state"] else 1))
                coords, label_from = [], None
            if s in dfa.final:
                break
        return out

    def batch(self, images: List, texts: List[str], suffixes: Optional[List[str]] = None) -> dict:
        """Several (image, prompt) pairs as one right-padded batch for ``generate`` (the reference handles one pair,
        its ``__call__`` asserts so): each pair goes through ``__call__`` alone -- so every row's ids are exactly its
        single-request ids, quirks included -- and the rows are padded on the right with the tokenizer's pad id to
        the longest.  Returns stacked ``pixel_values`` [B][3][S][S], ``input_ids`` [B][L] and ``attention_mask``
        [B][L] (ones over a row's own tokens, zeros over its padding); ``generate`` then gives every row what it
        gives that pair alone.

        suffixes (one answer per pair, for ``score``): row b is its single-request ids followed by the tokenised
        answer and ``<eos>``, and the result also holds ``token_type_ids`` [B][L]: 0 over the prompt row, 1 over the
        answer and its ``<eos>``, 0 over the padding.  Without suffixes the result is what it was."""
        if len(images) != len(texts) or not len(images):
            raise ValueError(f"batch: {len(images)} images for {len(texts)} prompts (need one prompt per image)")
        if suffixes is not None and len(suffixes) != len(texts):
            raise ValueError(f"batch: {len(suffixes)} suffixes for {len(texts)} prompts (need one answer per prompt)")
        pad = self.tokenizer.pad_token_id
        if pad is None:
            raise ValueError("batch: the tokenizer has no pad token to pad the shorter prompts with")
        rows = [self([im], [tx]) for im, tx in zip(images, texts)]
        tails = [[] for _ in rows]
        if suffixes is not None:
            eos = self.tokenizer.eos_token_id
            if eos is None:
                raise ValueError("batch: the tokenizer has no eos token to end the answers with")
            tails = [list(self.tokenizer(sx, add_special_tokens=False)["input_ids"]) + [eos] for sx in suffixes]
        L = max(r["input_ids"].shape[1] + len(t) for r, t in zip(rows, tails))
        ids = torch.full((len(rows), L), pad, dtype=rows[0]["input_ids"].dtype)
        mask = torch.zeros(len(rows), L, dtype=rows[0]["attention_mask"].dtype)
        types = torch.zeros(len(rows), L, dtype=rows[0]["input_ids"].dtype)
        for b, (r, t) in enumerate(zip(rows, tails)):
            n = r["input_ids"].shape[1]
            ids[b, :n] = r["input_ids"][0]
            mask[b, :n] = r["attention_mask"][0]
            if t:
                ids[b, n:n + len(t)] = torch.tensor(t, dtype=ids.dtype)
                mask[b, n:n + len(t)] = 1
                types[b, n:n + len(t)] = 1
        out = {"pixel_values": torch.cat([r["pixel_values"] for r in rows]), "input_ids": ids, "attention_mask": mask}
        if suffixes is not None:
            out["token_type_ids"] = types
        return out
