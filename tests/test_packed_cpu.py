"""Packed-sequence training without a GPU: the library exports the document-masked attention pair under ABI 4.12 and refuses
bad arguments before any launch; ops.document_layout; the model's stock branch under `document_ids` (packed rows equal the
documents run alone); every raising case; data.PackedDataset and ApertisTrainer(pack_sequences=True)."""
import ctypes
import json
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("apertis_attention_doc_fwd", "apertis_attention_fwd"), ("apertis_attention_doc_bwd", "apertis_attention_bwd"))


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _params(hdr, name):
    m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/apertis_hip.h"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_header_declares_and_binding_matches():
    from apertis_llm_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        hdr = f.read()
    for name, causal in PAIRS:
        assert hasattr(cdll, name), name
        params, base = _params(hdr, name), _params(hdr, causal)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, params)
        # the causal entry point's argument list plus the two int32 pointers, right after key_valid
        at = base.index("const int64_t *key_valid") + 1
        assert params == base[:at] + ["const int32_t *doc_start", "const int32_t *doc_end"] + base[at:]
        cargs = list(_lib.SIGNATURES[causal][1])
        assert list(argtypes) == cargs[:at] + [ctypes.c_void_p, ctypes.c_void_p] + cargs[at:]
    assert _lib.ABI_VERSION == (4 << 16) | 12 and int(_lib.load().apertis_abi_version()) == (4 << 16) | 12
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", hdr)


# ------------------------------------------------------------------------------------------------ refusals
# non-null, 16-byte aligned stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000


def _fwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, kv=None, start=P, end=P, out=P, lse=P, q_rs=192, k_rs=192, v_rs=192, o_rs=192, B=2, L=5, H=3, D=64,
                p=0.0, seed=0, dt=BF16), **kw}
    doc = (a["start"], a["end"]) if "doc" in name else ()
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["kv"], *doc, a["out"], a["o_rs"],
                                 a["lse"], a["B"], a["L"], a["H"], a["D"], a["p"], a["seed"], a["dt"], None)


def _bwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, out=P, dout=P, lse=P, kv=None, start=P, end=P, ws=P, dq=P, dk=P, dv=P, q_rs=192, k_rs=192, v_rs=192,
                o_rs=192, do_rs=192, d_rs=192, B=2, L=5, H=3, D=64, p=0.0, seed=0, dt=BF16), **kw}
    doc = (a["start"], a["end"]) if "doc" in name else ()
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["out"], a["o_rs"], a["dout"], a["do_rs"],
                                 a["lse"], a["kv"], *doc, a["ws"], a["dq"], a["dk"], a["dv"], a["d_rs"], a["B"], a["L"], a["H"],
                                 a["D"], a["p"], a["seed"], a["dt"], None)


def _refusals(call, ptrs, strides):
    got = [(f"null {n}", call(**{n: None})) for n in ptrs]
    got += [(f"p {p}", call(p=p)) for p in (-0.1, 1.0, 1.5, float("nan"))]
    got += [("D 32", call(D=32, **{s: 96 for s in strides}))]
    got += [("fp16", call(dt=2))]
    got += [("B*H 65536", call(B=16384, H=4, D=64, **{s: 256 for s in strides}))]
    got += [(f"misaligned {s}", call(**{s: 196})) for s in strides]            # bf16: 392-byte rows
    got += [(f"misaligned {n}", call(**{n: P + 8})) for n in ptrs]
    return dict(got)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    fs, bs = ("q_rs", "k_rs", "v_rs", "o_rs"), ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "d_rs")
    fp, bp = ("q", "k", "v", "out", "lse"), ("q", "k", "v", "out", "dout", "lse", "ws", "dq", "dk", "dv")
    for (doc, causal), call, ptrs, strides in zip(PAIRS, (_fwd, _bwd), (fp, bp), (fs, bs)):
        got = _refusals(lambda **kw: call(doc, **kw), ptrs, strides)
        want = _refusals(lambda **kw: call(causal, **kw), ptrs, strides)
        assert got == want, (doc, got, want)                                   # the causal pair's checks and codes
        assert all(got[f"null {n}"] == ERR_ARG for n in ptrs) and got["fp16"] == ERR_ARG
        assert got["D 32"] == ERR_UNSUPPORTED and got["B*H 65536"] == ERR_UNSUPPORTED
        assert all(got[f"misaligned {s}"] == ERR_UNSUPPORTED for s in strides)
        # the layout pointers: null is an argument error, whatever else is asked, work or no work
        assert call(doc, start=None) == ERR_ARG and call(doc, end=None) == ERR_ARG
        assert call(doc, L=0, start=None) == ERR_ARG and call(doc, B=0, end=None) == ERR_ARG
        assert call(doc, B=0) == OK and call(doc, L=0) == OK


# ------------------------------------------------------------------------------------------------ layout
def test_document_layout_values_and_errors():
    from apertis_llm_amd import ops
    ids = torch.tensor([[3, 3, 3, 4, 9, 9, 9], [0, 0, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6]])
    lay = ops.document_layout(ids)
    assert lay.start.dtype == torch.int32 and lay.end.dtype == torch.int32 and lay.positions.dtype == torch.int64
    assert lay.start.tolist() == [[0, 0, 0, 3, 4, 4, 4], [0] * 7, list(range(7))]
    assert lay.end.tolist() == [[3, 3, 3, 4, 7, 7, 7], [7] * 7, list(range(1, 8))]
    assert lay.positions.tolist() == [[0, 1, 2, 0, 0, 1, 2], list(range(7)), [0] * 7]
    assert lay.pairs == (6 + 1 + 6) + 28 + 7
    assert lay.start.is_contiguous() and lay.end.is_contiguous()
    one = ops.document_layout(torch.zeros(1, 1, dtype=torch.long))
    assert (one.start.tolist(), one.end.tolist(), one.pairs) == ([[0]], [[1]], 1)
    with pytest.raises(ValueError):
        ops.document_layout(torch.tensor([[0, 0, 1, 0]]))                      # ids that decrease
    with pytest.raises(ValueError):
        ops.document_layout(torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(ValueError):
        ops.document_layout(torch.tensor([0, 0, 1]))                           # not [B, L]
    with pytest.raises(ValueError):
        ops.document_layout(torch.tensor([[0.0, 1.0]]))
    for name in ("document_layout", "document_attention", "DocumentLayout"):
        assert hasattr(ops, name), name
    x = torch.zeros(1, 4, 128)
    with pytest.raises(ops.ApertisHipError):                                   # a CPU tensor: no fallback
        ops.document_attention(x, x, x, 2, ops.document_layout(torch.zeros(1, 4, dtype=torch.long)))


# ------------------------------------------------------------------------------------------------ model, stock path
def _model(A, **kw):
    base = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                attention_type="standard_mha", position_embedding_type="rotary", max_position_embeddings=64,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    torch.manual_seed(0)
    return A.ApertisForCausalLM(A.ApertisConfig(**base))


LENS = ([5, 1, 10], [16])


def _packed_batch():
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(4, 64, (2, 16), generator=gen)
    docs = torch.stack([torch.repeat_interleave(torch.arange(len(l)), torch.tensor(l)) for l in LENS])
    return ids, docs


@pytest.mark.parametrize("pos", ["rotary", "absolute"])
def test_stock_path_packed_equals_documents_alone(pos):
    """fp32, 1e-5: the arithmetic is identical apart from masked terms (exp of finfo.min differences is exactly zero)."""
    import apertis_llm_amd as A
    model = _model(A, position_embedding_type=pos).eval()
    ids, docs = _packed_batch()
    labels = ids.clone()
    with torch.no_grad():
        loss, logits = model(input_ids=ids, labels=labels, document_ids=docs)[:2]
        num, den = 0.0, 0
        for b, lens in enumerate(LENS):
            at = 0
            for n in lens:
                sl = slice(at, at + n)
                li, lg = model(input_ids=ids[b:b + 1, sl], labels=labels[b:b + 1, sl])[:2]
                torch.testing.assert_close(logits[b, sl], lg[0], rtol=1e-5, atol=1e-5 * float(lg.abs().max()))
                if n > 1:
                    num, den = num + float(li) * (n - 1), den + (n - 1)
                at += n
        assert abs(float(loss) - num / den) <= 1e-5 * abs(num / den)
        # the label of a document's first token is never a target: changing it changes nothing
        changed = labels.clone()
        changed[0, 5], changed[0, 6] = 7, 9
        assert float(model(input_ids=ids, labels=changed, document_ids=docs)[0]) == float(loss)
        # explicit position_ids are respected: the model's own give the same numbers, others do not
        lay = A.ops.document_layout(docs)
        same = model(input_ids=ids, document_ids=docs, position_ids=lay.positions)[1]
        other = model(input_ids=ids, document_ids=docs, position_ids=lay.positions + 3)[1]
        assert torch.equal(same, logits) and not torch.equal(other, logits)
        # all-ones attention_mask is accepted and changes nothing
        assert torch.equal(model(input_ids=ids, document_ids=docs, attention_mask=torch.ones_like(ids))[1], logits)


def test_packed_gradients_flow_through_checkpointing_on_the_stock_path():
    import apertis_llm_amd as A
    model = _model(A).train()
    ids, docs = _packed_batch()
    grads = []
    for ckpt in (False, True):
        model.model.gradient_checkpointing = ckpt
        model.zero_grad(set_to_none=True)
        model(input_ids=ids, labels=ids, document_ids=docs)[0].backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and grads[0]
    for n in grads[0]:
        torch.testing.assert_close(grads[1][n], grads[0][n], rtol=1e-5, atol=1e-7, msg=n)


def test_every_raising_case():
    import apertis_llm_amd as A
    model = _model(A).eval()
    ids, docs = _packed_batch()
    mask = torch.ones_like(ids)
    mask[0, 12:] = 0
    with torch.no_grad():
        past = model(input_ids=ids[:, :4], use_cache=True)[4]
        bad = [dict(attention_mask=mask), dict(past_key_values=past), dict(use_cache=True),
               dict(pixel_values=torch.zeros(2, 3, 8, 8)), dict(document_ids=docs[:, :8]),
               dict(document_ids=docs.flip(1))]
        for kw in bad:
            with pytest.raises(ValueError):
                model(**{**dict(input_ids=ids, document_ids=docs), **kw})
            with pytest.raises(ValueError):
                model.model(**{**dict(input_ids=ids, document_ids=docs), **kw})
        with pytest.raises(ValueError):
            model.generate(input_ids=ids, document_ids=docs, max_new_tokens=2)
        ssm = _model(A, attention_type="selective_ssm").eval()
        with pytest.raises(ValueError):
            ssm(input_ids=ids, document_ids=docs)
        # the configuration's use_cache default does not apply to a packed forward
        assert model.config.use_cache and model(input_ids=ids, document_ids=docs)[4] is None
    assert "document_ids" not in model.config.to_dict() and "pack_sequences" not in model.config.to_dict()


# ------------------------------------------------------------------------------------------------ PackedDataset
def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return str(p)


def _pretrain(tmp_path, lengths, max_length=8, name="d.jsonl"):
    from apertis_llm_amd import data as D
    words = list("abcdefgh")
    lines = [json.dumps({"text": " ".join(words[(i + j) % 8] for j in range(n))}) for i, n in enumerate(lengths)]
    vocab = {c: i + 4 for i, c in enumerate(words)}
    return D.ApertisPretrainDataset(_write(tmp_path, name, "\n".join(lines)), vocab, 16, max_length=max_length)


def test_packed_dataset_plan_and_rows(tmp_path):
    from apertis_llm_amd import data as D
    lengths = [5, 3, 8, 2, 0, 4, 1, 12]                       # 12 is truncated to 8 by the wrapped dataset; 0 is left out
    src = _pretrain(tmp_path, lengths)
    ds = D.PackedDataset(src, 8, 0)
    assert ds.lengths == [5, 3, 8, 2, 0, 4, 1, 8] and max(ds.lengths) <= ds.max_length
    assert ds.rows == [[0, 1], [2], [3, 5, 6], [7]] and len(ds) == 4 < len(src)      # first fit, index order
    assert D.PackedDataset(src, 8, 0).rows == ds.rows          # deterministic
    seen = []
    for r in range(len(ds)):
        row = ds[r]
        assert set(row) == {"input_ids", "labels", "document_ids"}
        assert all(t.shape == (8,) and t.dtype == torch.int64 for t in row.values())
        docs = row["document_ids"]
        assert bool((docs[1:] >= docs[:-1]).all())
        at = 0
        for d, i in enumerate(ds.rows[r]):
            n = ds.lengths[i]
            assert row["input_ids"][at:at + n].tolist() == src[i]["input_ids"][:n].tolist()          # in order, one document
            assert row["labels"][at:at + n].tolist() == src[i]["labels"][:n].tolist()                # labels carried over
            assert docs[at:at + n].tolist() == [d] * n
            seen.append(i)
            at += n
        # the tail: pad tokens, ignored labels, a document id of its own
        assert row["input_ids"][at:].tolist() == [0] * (8 - at) and row["labels"][at:].tolist() == [-100] * (8 - at)
        assert docs[at:].tolist() == [len(ds.rows[r])] * (8 - at)
    assert sorted(seen) == [i for i, n in enumerate(ds.lengths) if n]                # every source item exactly once
    assert ds[0]["document_ids"].tolist() == [0] * 5 + [1] * 3 and ds[2]["document_ids"].tolist() == [0, 0, 1, 1, 1, 1, 2, 3]
    # an item longer than max_length cannot come from the wrapped datasets (they truncate): packing into shorter rows raises
    with pytest.raises(ValueError):
        D.PackedDataset(src, 6, 0)

    class _Img(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {**src[0], "pixel_values": torch.zeros(3, 4, 4)}
    with pytest.raises(ValueError):
        D.PackedDataset(_Img(), 8, 0)


def test_packed_dataset_keeps_fine_tuning_labels(tmp_path):
    from apertis_llm_amd import data as D
    vocab = {w: i + 4 for i, w in enumerate("User: Assistant: a b c d".split())}
    lines = [json.dumps({"instruction": "a b", "output": "c"}), json.dumps({"instruction": "a", "output": "c d"})]
    src = D.ApertisFineTuneDataset(_write(tmp_path, "ft.jsonl", "\n".join(lines)), vocab, max_length=16, is_hf_tokenizer=False,
                                   model_config_vocab_size=16, model_config_eos_token_id=0, model_config_pad_token_id=0,
                                   model_config_unk_token_id=3)
    ds = D.PackedDataset(src, 16, 0)
    assert len(ds) == 1 and ds.rows == [[0, 1]]
    row, at = ds[0], 0
    for i in (0, 1):
        item, n = src[i], ds.lengths[i]
        # the closing EOS equals the pad id here: the attention mask drops it, its label keeps it inside the document
        assert int(item["attention_mask"].sum()) == n - 1 and int(item["labels"][n - 1]) == 0
        assert row["labels"][at:at + n].tolist() == item["labels"][:n].tolist()
        assert int((row["labels"][at:at + n] == -100).sum()) >= 3                     # the prompt part stays masked
        at += n


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_packs_sequences(tmp_path):
    import apertis_llm_amd as A
    from apertis_llm_amd import data as D
    from apertis_llm_amd.trainer import ApertisTrainer, build_from_config
    train = _pretrain(tmp_path, [3, 5, 2, 6, 4, 1, 7, 3, 2, 5], max_length=16)
    val = _pretrain(tmp_path, [4, 4, 9], max_length=16, name="v.jsonl")
    model = _model(A, vocab_size=16)
    t = ApertisTrainer(model, train, val, output_dir=str(tmp_path / "out"), batch_size=2, learning_rate=1e-2, num_epochs=2,
                       gradient_accumulation_steps=1, fp16=False, device="cpu", checkpoint_steps=0, shuffle=False, num_workers=0,
                       pack_sequences=True)
    assert isinstance(t.train_dataset, D.PackedDataset) and isinstance(t.val_dataset, D.PackedDataset)
    assert len(t.train_dataset) == 3 < len(train) and len(t.val_dataset) == 2          # fewer rows than items
    assert "attention_mask" not in next(iter(t.train_dataloader))
    t.train()
    assert len(t.history["loss"]) == 4 and all(torch.isfinite(torch.tensor(t.history["loss"])))     # 2 steps per epoch
    assert t.history["loss"][-1] <= t.history["loss"][0] and len(t.history["val_loss"]) == 2
    # off by default; not for a model whose state would run across documents
    t0 = ApertisTrainer(_model(A, vocab_size=16), train, None, output_dir=str(tmp_path / "o0"), fp16=False, device="cpu",
                        num_workers=0)
    assert t0.train_dataset is train and t0.pack_sequences is False
    with pytest.raises(ValueError):
        ApertisTrainer(_model(A, vocab_size=16, attention_type="selective_ssm"), train, None, output_dir=str(tmp_path / "o1"),
                       fp16=False, device="cpu", num_workers=0, pack_sequences=True)
    # the configuration file's switch
    vpath = _write(tmp_path, "vocab.json", json.dumps({c: i + 4 for i, c in enumerate("abcdefgh")}))
    cfg = {"data_config": {"tokenizer_path": vpath, "train_data_path": train.data_path, "max_length": 16},
           "model_config": {"attention_type": "standard_mha", "config_overrides": {
               "hidden_size": 128, "num_hidden_layers": 1, "num_attention_heads": 2, "intermediate_size": 128}},
           "training_config": {"output_dir": str(tmp_path / "o2"), "device": "cpu", "fp16": False, "pack_sequences": True}}
    tc = build_from_config(cfg, num_workers=0)
    assert isinstance(tc.train_dataset, D.PackedDataset) and tc.train_dataset.rows == t.train_dataset.rows
    cfg["training_config"].pop("pack_sequences")
    assert not isinstance(build_from_config(cfg, num_workers=0).train_dataset, D.PackedDataset)
