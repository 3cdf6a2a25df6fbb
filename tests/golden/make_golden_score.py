#!/usr/bin/env python3
"""Generate tests/golden/score.npz from the REFERENCE model's own ``forward(labels=...)`` (chatglm_q/model.py:384-390).

Like make_golden.py this script imports the reference from its read-only checkout, feeds it seeded inputs and stores data
only - here ids, attention masks, labels and what the reference computed from them: the scalar loss and, per token,
``log_softmax(logits.float())`` gathered at the shifted labels (0 where the label is -100).  No logits, no weights: the tiny
cases load the state dict already stored in tiny_model.npz, the real-width cases fill the reference model with
tests/_golden.py::fill_seeded_ (a pure function of key and shape, which takes the 65024-wide head as it takes any other).

Cases (labels follow the reference tokenizer's ``return_labels``, chatglm_q/tokenizer.py:138-142: the ids, -100 at pads):
  tiny/f32, tiny/f16   the tiny config, batch 3 left padded, row 1 with a -100 "prompt" span in its labels
  real/b4              REAL_DIM_CONFIG (6B layer width, 2 layers, vocabulary 1024), 4 x 40 ids, lengths 40 / 31 / 12 / 26
  real/long            the same model, 1 x 300 ids (more than one attention window)
  real/v65k            the same config with vocab_size = 65024, 2 x 48 ids, lengths 48 / 35

Usage:  CHATGLM_Q_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_score.py
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


def left_padded(gen, V, S, lens):
    ids = torch.randint(0, V, (len(lens), S), generator=gen)
    attn = torch.zeros(len(lens), S, dtype=torch.long)
    for b, n in enumerate(lens):
        attn[b, S - n:] = 1
        ids[b, : S - n] = 0
    labels = torch.where(attn.bool(), ids, torch.full_like(ids, -100))
    return ids, attn, labels


def record(d, name, m, ids, attn, labels):
    with torch.no_grad():
        loss, logits, _ = m(input_ids=ids, attention_mask=attn, labels=labels)
    tgt = labels[:, 1:]
    lsm = torch.log_softmax(logits[:, :-1].float(), dim=-1)
    lp = lsm.gather(2, tgt.clamp(min=0)[..., None])[..., 0]
    lp = torch.where(tgt == -100, torch.zeros_like(lp), lp)
    assert bool(((tgt != -100).sum(dim=1) > 0).all()), "every row needs a scored target"
    mean = -(lp.double().sum() / (tgt != -100).sum())
    assert abs(float(mean) - float(loss)) <= 1e-5 * abs(float(loss)), (float(mean), float(loss))   # the two records agree
    d[name + "/ids"] = ids.numpy()
    d[name + "/attention_mask"] = attn.numpy()
    d[name + "/labels"] = labels.numpy()
    d[name + "/loss"] = np.array(float(loss), dtype=np.float32)
    d[name + "/logprobs"] = lp.numpy().astype(np.float32)
    print(name, tuple(ids.shape), "loss", float(loss), "scored", int((tgt != -100).sum()))


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
        gen = torch.Generator().manual_seed(9100)
        ids, attn, labels = left_padded(gen, cfg.vocab_size, 14, [14, 9, 11])
        labels[1, 5:9] = -100                                   # row 1 (tokens from column 5 on): its first 4 tokens are a prompt
        record(d, f"tiny/{dt}", m, ids, attn, labels)


def gen_real(d):
    torch.set_num_threads(8)
    for vocab, cases in ((G.REAL_DIM_CONFIG["vocab_size"], (("real/b4", 40, [40, 31, 12, 26]), ("real/long", 300, [300]))),
                         (65024, (("real/v65k", 48, [48, 35]),))):
        cfg = refm.ChatGLM2Config(**dict(G.REAL_DIM_CONFIG, vocab_size=vocab))
        m = refl.create_quant_int4_model(cfg, dtype=torch.float16)
        G.fill_seeded_(m.state_dict(), G.REAL_DIM_SEED)
        m.eval()
        gen = torch.Generator().manual_seed(9200 + vocab)
        for name, S, lens in cases:
            record(d, name, m, *left_padded(gen, vocab, S, lens))
        del m


if __name__ == "__main__":
    d = {}
    gen_tiny(d)
    gen_real(d)
    d["seed"] = np.array([G.REAL_DIM_SEED])
    np.savez_compressed(os.path.join(OUT, "score.npz"), **d)
    print("wrote score.npz", os.path.getsize(os.path.join(OUT, "score.npz")), "bytes")
