"""Tokenizers for the serving engine.

* ``HFTokenizer``: a checkpoint's ``tokenizer.json`` through the ``tokenizers`` library, with the
  chat template from ``tokenizer_config.json`` (Jinja) when present.
* ``ByteTokenizer``: UTF-8 bytes as token ids (offset by the special ids) for built-in
  random-weight configs — there is no network to fetch a vocabulary, and a random model's outputs
  carry no meaning anyway; it keeps the OpenAI API path (text in, text out, token counts) whole.

Both expose ``encode``, ``decode``, ``apply_chat_template``, ``eos_token_ids`` and ``bos_token_id``.
"""

from __future__ import annotations

import json
import os


def _llama3_chat(messages, add_generation_prompt=True) -> str:
    """The Llama-3 instruct chat format (used when a checkpoint ships no template)."""
    out = "<|begin_of_text|>"
    for m in messages:
        out += f"<|start_header_id|>{m['role']}<|end_header_id|>\n\n{_content(m)}<|eot_id|>"
    if add_generation_prompt:
        out += "<|start_header_id|>assistant<|end_header_id|>\n\n"
    return out


def _content(m) -> str:
    c = m.get("content", "")
    if isinstance(c, list):  # OpenAI content parts
        return "".join(p.get("text", "") for p in c if isinstance(p, dict))
    return c or ""


class ByteTokenizer:
    PAD, BOS, EOS = 0, 1, 2
    OFFSET = 3

    def __init__(self, vocab_size: int):
        self.vocab_size = vocab_size
        self.bos_token_id = self.BOS
        self.eos_token_ids = (self.EOS,)

    def encode(self, text: str, add_bos: bool = True) -> list[int]:
        ids = [b + self.OFFSET for b in text.encode("utf-8")]
        return ([self.BOS] if add_bos else []) + ids

    def decode(self, ids) -> str:
        # ids outside the byte range (a random model samples the whole vocabulary) map onto bytes
        bs = bytes((i - self.OFFSET) % 256 for i in ids if i >= self.OFFSET)
        return bs.decode("utf-8", errors="replace")

    def token_bytes(self) -> list[bytes]:
        """The bytes every id contributes to ``decode`` (structured outputs walk them through a DFA)."""
        return [b"" if i < self.OFFSET else bytes([(i - self.OFFSET) % 256]) for i in range(self.vocab_size)]

    def apply_chat_template(self, messages, add_generation_prompt=True) -> str:
        out = ""
        for m in messages:
            out += f"<{m['role']}>{_content(m)}\n"
        return out + ("<assistant>" if add_generation_prompt else "")


def _gpt2_unicode_to_byte() -> dict:
    """Inverse of the GPT-2 byte-to-unicode table the ByteLevel pre-tokenizer / decoder uses."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[chr(b)] = b
        else:
            table[chr(256 + n)] = b
            n += 1
    return table


def _decoder_kinds(dec) -> set:
    """The decoder types named in a ``tokenizer.json`` decoder entry (a Sequence is flattened)."""
    if not isinstance(dec, dict):
        return set()
    if dec.get("type") == "Sequence":
        return set().union(*[_decoder_kinds(d) for d in dec.get("decoders", [])]) if dec.get("decoders") else set()
    return {dec.get("type")}


class HFTokenizer:
    def __init__(self, path: str):
        from tokenizers import Tokenizer

        self.tok = Tokenizer.from_file(os.path.join(path, "tokenizer.json"))
        self.vocab_size = self.tok.get_vocab_size()
        cfg = {}
        p = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(p):
            with open(p) as f:
                cfg = json.load(f)
        self.chat_template = cfg.get("chat_template")
        self.bos_token_id = self._id(cfg.get("bos_token"))
        eos = [self._id(cfg.get("eos_token"))]
        for extra in ("<|eot_id|>", "<|end_of_text|>"):
            eos.append(self.tok.token_to_id(extra))
        self.eos_token_ids = tuple(sorted({e for e in eos if e is not None}))
        self._bos_text = cfg.get("bos_token") if isinstance(cfg.get("bos_token"), str) else None

    def _id(self, tok):
        if isinstance(tok, dict):
            tok = tok.get("content")
        return self.tok.token_to_id(tok) if isinstance(tok, str) else None

    def encode(self, text: str, add_bos: bool = True) -> list[int]:
        ids = self.tok.encode(text, add_special_tokens=False).ids
        if add_bos and self.bos_token_id is not None and (not ids or ids[0] != self.bos_token_id):
            ids = [self.bos_token_id] + ids
        return ids

    def decode(self, ids) -> str:
        return self.tok.decode(list(ids), skip_special_tokens=True)

    def token_bytes(self) -> list[bytes]:
        """The bytes every id contributes to ``decode``, read off the decoder ``tokenizer.json``
        names: ByteLevel (Llama-3, Qwen2) inverts the GPT-2 byte-to-unicode table; Metaspace /
        ByteFallback (Llama-2, Mistral) turns ``▁`` into a space and ``<0xNN>`` into that byte.  Added
        and special tokens are empty.  ValueError for any other decoder."""
        spec = json.loads(self.tok.to_str())
        kinds = _decoder_kinds(spec.get("decoder"))
        vocab = self.tok.get_vocab(with_added_tokens=True)
        added = {t["id"] for t in spec.get("added_tokens") or []}
        out = [b""] * (max(vocab.values()) + 1 if vocab else 0)
        if "ByteLevel" in kinds:
            inv = _gpt2_unicode_to_byte()
            for text, i in vocab.items():
                if i not in added:
                    try:
                        out[i] = bytes(inv[c] for c in text)
                    except KeyError:
                        raise ValueError(f"token {i} ({text!r}) is not in the ByteLevel alphabet") from None
        elif kinds & {"Metaspace", "ByteFallback"}:
            for text, i in vocab.items():
                if i in added:
                    continue
                if len(text) == 6 and text.startswith("<0x") and text.endswith(">") and "ByteFallback" in kinds:
                    try:
                        out[i] = bytes([int(text[3:5], 16)])
                        continue
                    except ValueError:
                        pass
                out[i] = text.replace("▁", " ").encode("utf-8")
        else:
            raise ValueError(f"structured outputs need a ByteLevel or Metaspace / ByteFallback tokenizer; this one "
                             f"decodes with {sorted(k for k in kinds if k) or 'no decoder'}")
        return out

    def apply_chat_template(self, messages, add_generation_prompt=True) -> str:
        if not self.chat_template:
            return _llama3_chat(messages, add_generation_prompt)
        import jinja2

        env = jinja2.Environment(trim_blocks=True, lstrip_blocks=True)
        env.globals["raise_exception"] = lambda msg: (_ for _ in ()).throw(ValueError(msg))
        return env.from_string(self.chat_template).render(
            messages=messages, add_generation_prompt=add_generation_prompt, bos_token=self._bos_text or "")


def load_tokenizer(model_path: str | None, vocab_size: int):
    if model_path and os.path.exists(os.path.join(model_path, "tokenizer.json")):
        return HFTokenizer(model_path)
    return ByteTokenizer(vocab_size)
