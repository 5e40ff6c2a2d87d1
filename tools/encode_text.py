"""Text prompts -> the CLIP text-encoding files the reference's datasets ship, computed on the device library
(asva_amd/text_encoder.py):

    python tools/encode_text.py --sd15 ./pretrained/stable-diffusion-v1-5 --out class_clip_text_encodings_stable-diffusion-v1-5.pt \\
        [--null-out openai-clip-l_null_text_encoding.pt] "dog barking" "hammering" ...

--out holds a dict that maps each prompt to its (77, 768) f32 encoding; --null-out holds the encoding of "" (the unconditional branch
of text guidance).  --sd15 is a folder with tokenizer/ (vocab.json, merges.txt) and text_encoder/ (config.json + weights).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sd15", required=True, help="Stable Diffusion 1.5 folder (tokenizer/ and text_encoder/)")
    ap.add_argument("--out", required=True, help="file for {prompt: (L, C) f32 encoding}")
    ap.add_argument("--null-out", default="", help="file for the encoding of the empty prompt")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("prompts", nargs="*")
    args = ap.parse_args(argv)
    if not args.prompts and not args.null_out:
        ap.error("no prompts and no --null-out: nothing to do")

    import torch

    from asva_amd.text_encoder import CLIPTextModel, CLIPTokenizer

    tokenizer = CLIPTokenizer.from_pretrained(args.sd15, subfolder="tokenizer")
    encoder = CLIPTextModel.from_pretrained(args.sd15, subfolder="text_encoder").to(args.device)

    def encode(texts):
        ti = tokenizer(texts, padding="max_length", max_length=tokenizer.model_max_length, truncation=True, return_tensors="pt")
        return encoder(ti.input_ids)[0].cpu()

    if args.prompts:
        enc = encode(args.prompts)
        torch.save({p: enc[i].clone() for i, p in enumerate(args.prompts)}, args.out)
        print(f"{args.out}: {len(args.prompts)} prompts, each {tuple(enc.shape[1:])} {enc.dtype}")
    if args.null_out:
        null = encode([""])[0].clone()
        torch.save(null, args.null_out)
        print(f"{args.null_out}: {tuple(null.shape)} {null.dtype}")


if __name__ == "__main__":
    main()
