#!/usr/bin/env python3
"""Generate tests/golden/batch_generate.npz: the REFERENCE model's greedy continuation of left-padded batches.

Like make_golden_score.py this script imports the reference from its read-only checkout, feeds it seeded inputs and stores data
only.  A batched continuation is what the reference's ``forward`` defines for left-padded ``input_ids`` + ``attention_mask``
with ``past_key_values`` (chatglm_q/model.py:297-318,329-392): one forward over the prompts, then one forward per step over the
fed-back argmax tokens, the mask grown by one column of ones per step.  Stored per case: ids and attention mask, the reference's
tokens (B, T), every step's last-position logits (B, T, V) (fp32 for tiny, fp16 for real width) and the top-2 margin per
(row, step) - the gap between the largest and the second largest logit, which bounds how much noise a token survives.

Cases (prompt ids: ``torch.Generator().manual_seed(seed)``, ``randint(0, V, (B, S))``, pads 0 on the left):
  tiny/f32, tiny/f16   tiny_model.npz, prompt lengths 12 / 7 / 10, seed 9300, 16 greedy steps
  real/b4              REAL_DIM_CONFIG filled by fill_seeded_ (6B layer width, 2 layers, vocabulary 1024), fp16, prompt lengths
                       24 / 17 / 9 / 20, seed 9408, 12 greedy steps

Usage:  CHATGLM_Q_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batch_generate.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("CHATGLM_Q_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "chatglm_q")):
    sys.exit("set CHATGLM_Q_REFERENCE to the reference checkout (the folder that holds chatglm_q/)")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))                        # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))       # repository root (tests/_golden.py imports oracle/)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _golden as G  # noqa: E402
from chatglm_q import loader as refl  # noqa: E402
from chatglm_q import model as refm  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16}


def left_padded(seed, V, lens):
    S = max(lens)
    ids = torch.randint(0, V, (len(lens), S), generator=torch.Generator().manual_seed(seed))
    attn = torch.zeros(len(lens), S, dtype=torch.long)
    for b, n in enumerate(lens):
        attn[b, S - n:] = 1
        ids[b, : S - n] = 0
    return ids, attn


def record(d, name, m, ids, attn, steps, logits_dtype):
    B = ids.shape[0]
    toks, steps_logits = [], []
    mask, inp, past = attn, ids, None
    with torch.no_grad():
        for t in range(steps):
            _, out, past = m(input_ids=inp, attention_mask=mask, past_key_values=past)
            last = out[:, -1].float()
            nxt = last.argmax(dim=-1)
            toks.append(nxt)
            steps_logits.append(last)
            inp = nxt[:, None]
            mask = torch.cat([mask, torch.ones(B, 1, dtype=mask.dtype)], dim=1)
    tokens = torch.stack(toks, dim=1)                           # (B, T)
    logits = torch.stack(steps_logits, dim=1)                   # (B, T, V) fp32
    top2 = logits.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    d[name + "/ids"] = ids.numpy()
    d[name + "/attention_mask"] = attn.numpy()
    d[name + "/tokens"] = tokens.numpy()
    d[name + "/logits"] = logits.to(logits_dtype).numpy()
    d[name + "/margin"] = margin.numpy().astype(np.float32)
    mg = margin.flatten()
    print(name, tuple(ids.shape), "steps", steps, "smallest top-2 margin %.4f" % float(mg.min()),
          "below 0.03: %d, below 0.05: %d of %d" % (int((mg < 0.03).sum()), int((mg < 0.05).sum()), mg.numel()))


def gen_tiny(d):
    torch.set_num_threads(1)
    Z = G.load("tiny_model.npz")
    c = [int(v) for v in Z["config"]]
    cfg = refm.ChatGLM2Config(hidden_size=c[0], inner_hidden_size=c[1], head_hidden_size=c[2], num_multi_query_groups=c[3],
                              num_attention_heads=c[4], num_layers=c[5], vocab_size=c[6], max_sequence_length=c[7])
    for dt in ("f32", "f16"):
        m = refl.create_quant_int4_model(cfg, dtype=DT[dt])
        sd = m.state_dict()
        for k in sd:
            sd[k].copy_(torch.from_numpy(Z[f"{dt}/sd/{k}"]))
        m.eval()
        ids, attn = left_padded(9300, cfg.vocab_size, [12, 7, 10])
        record(d, f"tiny/{dt}", m, ids, attn, 16, torch.float32)


def gen_real(d):
    torch.set_num_threads(16)
    cfg = refm.ChatGLM2Config(**G.REAL_DIM_CONFIG)
    m = refl.create_quant_int4_model(cfg, dtype=torch.float16)
    G.fill_seeded_(m.state_dict(), G.REAL_DIM_SEED)
    m.eval()
    ids, attn = left_padded(9408, cfg.vocab_size, [24, 17, 9, 20])
    record(d, "real/b4", m, ids, attn, 12, torch.float16)


if __name__ == "__main__":
    d = {}
    gen_tiny(d)
    gen_real(d)
    d["seed"] = np.array([G.REAL_DIM_SEED])
    np.savez_compressed(os.path.join(OUT, "batch_generate.npz"), **d)
    print("wrote batch_generate.npz", os.path.getsize(os.path.join(OUT, "batch_generate.npz")), "bytes")
