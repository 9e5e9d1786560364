"""Image->text generation entry point — drop-in for the reference's ``inference.py``.

Same functions and CLI flags as inference.py:11-154 (``main``, ``test_inference``,
``_sample_top_p``, ``get_model_inputs``, ``move_inputs_to_device``); flags are parsed with
argparse in fire's ``--name value`` form (fire is not installed offline).  The token loop
keeps the reference's semantics — one model call per generated token, greedy argmax or
softmax(logits/T) + top-p sampling, stop at the tokenizer's EOS, print ``prompt + decoded`` —
but runs on the HIP engine: vision once, graph-replayed decode steps, sampling on the device.
There is no CPU path: ``--only_cpu True`` is rejected (the reference forces CPU at :127).
"""
from __future__ import annotations

import argparse
import sys

import torch

from modeling_gemma import KVCache  # noqa: F401  (re-exported like the reference's import)
from modeling_paligemma import PaliGemmaForConditionalGeneration
from pghip import ops
from processing_paligemma import PaliGemmaProcessor
from utils import load_hf_model


def move_inputs_to_device(model_inputs: dict, device: str):
    return {k: v.to(device) for k, v in model_inputs.items()}


def get_model_inputs(processor: PaliGemmaProcessor, prompt: str, image_file_path: str, device: str):
    from PIL import Image
    image = Image.open(image_file_path)
    return move_inputs_to_device(processor(text=[prompt], images=[image]), device)


def _sample_top_p(probs: torch.Tensor, p: float):
    """Top-p draw from a probability matrix (B, V) -> (B, 1) token ids (inference.py:90-106).

    Same filter (sorted-descending mass before a token <= p, renormalised) on the device; the
    draw is an inverse CDF with a fresh uniform per row (torch.multinomial's stream is not
    reproducible across devices anyway)."""
    if not probs.is_cuda:
        raise RuntimeError("_sample_top_p: HIP device only")
    B = probs.shape[0]
    logits = torch.log(probs.float().clamp_min(1e-38)).contiguous()
    out = torch.empty(B, dtype=torch.int64, device=probs.device)
    u = torch.rand(1, B, device=probs.device)
    ops.topp_sample(logits, out, u, temperature=1.0, top_p=float(p))
    return out.view(B, 1)


def detect_labels(detect: str) -> list:
    """The labels of a ``--detect "cat ; dog"`` argument."""
    labels = [lb.strip() for lb in str(detect).split(";")]
    if not labels or any(not lb for lb in labels):
        raise ValueError(f"--detect takes labels separated by ';', got {detect!r}")
    return labels


def detect_prompt(detect: str) -> str:
    """PaliGemma's detection prompt for a ``--detect`` argument: ``detect cat ; dog``."""
    return "detect " + " ; ".join(detect_labels(detect))


def choice_list(choices: str) -> list:
    """The answers of a ``--choices "yes|no|unsure"`` argument."""
    out = [c.strip() for c in str(choices).split("|")]
    if not out or any(not c for c in out):
        raise ValueError(f"--choices takes answers separated by '|', got {choices!r}")
    return out


def check_constraint_flags(detect=None, choices=None, num_beams: int = 1, prompt=None):
    """The flag conflicts of constrained decoding (ValueError, before any model is loaded): --detect and --choices
    exclude each other and --num_beams > 1 (the grammar does not follow a beam's parent map), and --detect builds its
    own prompt."""
    if detect is not None and choices is not None:
        raise ValueError("--detect and --choices are mutually exclusive")
    if (detect is not None or choices is not None) and num_beams != 1:
        raise ValueError("--detect / --choices constrain the greedy / sampling loop; they cannot be combined with "
                         "--num_beams > 1")
    if detect is not None and prompt is not None:
        raise ValueError("--detect builds the prompt itself (detect a ; b); drop --prompt")
    if detect is not None:
        detect_labels(detect)
    if choices is not None:
        choice_list(choices)


def test_inference(model: PaliGemmaForConditionalGeneration, processor: PaliGemmaProcessor, device: str,
                   prompt: str, image_file_path: str, max_tokens_to_generate: int, temperature: float,
                   top_p: float, do_sample: bool, num_beams: int = 1, detect: str = None, choices: str = None):
    """Generate until EOS or max_tokens_to_generate, then print prompt + decoded (inference.py:29-87).  num_beams > 1
    (not in the reference): beam search instead, the best hypothesis printed (greedy within the beams: do_sample,
    temperature and top_p do not apply).  detect ("cat ; dog", not in the reference): the prompt becomes ``detect cat ;
    dog``, the answer is constrained to boxes of those labels (PaliGemmaProcessor.detect_grammar) and the boxes are
    printed in pixels of the image; choices ("yes|no|unsure"): the answer is constrained to one of them."""
    check_constraint_flags(detect, choices, num_beams, prompt if detect is not None else None)
    grammar = None
    if detect is not None:
        prompt = detect_prompt(detect)
        grammar = processor.detect_grammar(detect_labels(detect), vocab=model.config.vocab_size)
    elif choices is not None:
        grammar = processor.choices_grammar(choice_list(choices), vocab=model.config.vocab_size)
    inputs = get_model_inputs(processor, prompt, image_file_path, device)
    if num_beams != 1:
        if do_sample:
            raise ValueError("--num_beams searches deterministically; drop --do_sample")
        res = model.generate_beam(inputs["input_ids"], inputs["pixel_values"], inputs["attention_mask"],
                                  max_new_tokens=max_tokens_to_generate, num_beams=num_beams,
                                  stop_token=processor.tokenizer.eos_token_id)
        ids = torch.tensor([res["sequences"][0][0]], dtype=torch.int64)
        print(prompt + processor.tokenizer.decode(ids[0], skip_special_tokens=True))
        return ids
    ids = model.generate(inputs["input_ids"], inputs["pixel_values"], inputs["attention_mask"],
                         max_new_tokens=max_tokens_to_generate, do_sample=do_sample, temperature=temperature,
                         top_p=top_p, stop_token=processor.tokenizer.eos_token_id, grammar=grammar)
    decoded = processor.tokenizer.decode(ids[0], skip_special_tokens=True)
    print(prompt + decoded)
    if detect is not None:
        from PIL import Image
        with Image.open(image_file_path) as im:
            width, height = im.size
        try:
            boxes = processor.parse_detections(ids[0], height, width, grammar=grammar)
        except ValueError as e:             # cut short by max_tokens_to_generate: nothing to parse
            print(f"no complete detection answer: {e}")
            return ids
        for d in boxes:
            y0, x0, y1, x1 = d["box"]
            print(f"{d['label']}: y {y0:.1f}..{y1:.1f}, x {x0:.1f}..{x1:.1f}")
        if not boxes:
            print("no detections")
    return ids


def main(model_path: str = None, prompt: str = None, image_file_path: str = None, max_tokens_to_generate: int = 100,
         temperature: float = 0.8, top_p: float = 0.9, do_sample: bool = False, only_cpu: bool = False,
         num_beams: int = 1, detect: str = None, choices: str = None):
    check_constraint_flags(detect, choices, num_beams, prompt)      # before anything is loaded
    if only_cpu:
        raise RuntimeError("this build has no CPU path (HIP kernels only); drop --only_cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible")
    device = "cuda"
    print("Device in use: ", device)
    print("Loading model")
    model, tokenizer = load_hf_model(model_path, device)
    model = model.to(device).eval()
    # resize + normalise on the device, bit-exact with PIL, for RGB, RGBA (the sample pic1.png), LA, L, P and 1 inputs;
    # any other mode takes the processor's host path
    processor = PaliGemmaProcessor(tokenizer, model.config.vision_config.num_image_tokens or
                                   model.config.text_config.num_image_tokens, model.config.vision_config.image_size,
                                   device=device)
    print("Running inference")
    with torch.no_grad():
        test_inference(model, processor, device, prompt, image_file_path, max_tokens_to_generate, temperature,
                       top_p, do_sample, num_beams=num_beams, detect=detect, choices=choices)


def _bool(s) -> bool:
    if isinstance(s, bool):
        return s
    return str(s).strip().lower() in ("1", "true", "yes", "y", "t")


def _cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model_path")
    ap.add_argument("--prompt")
    ap.add_argument("--image_file_path")
    ap.add_argument("--max_tokens_to_generate", type=int, default=100)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top_p", type=float, default=0.9)
    ap.add_argument("--do_sample", type=_bool, default=False)
    ap.add_argument("--only_cpu", type=_bool, default=False)
    ap.add_argument("--num_beams", type=int, default=1, help="beam search with this many beams (1: the greedy / "
                    "sampling loop)")
    ap.add_argument("--detect", default=None, help='labels to detect, "cat ; dog": the prompt becomes "detect cat ; '
                    'dog", the answer is constrained to <loc> boxes of these labels and the boxes are printed')
    ap.add_argument("--choices", default=None, help='a closed answer set, "yes|no|unsure": the answer is constrained '
                    "to one of them")
    a = ap.parse_args(argv)
    main(**vars(a))


if __name__ == "__main__":
    _cli(sys.argv[1:])
