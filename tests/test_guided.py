"""Structured outputs: the grammar compiler (regex / choice / JSON schema -> byte-level DFA), the
token byte tables, the mask (reference on the CPU, HIP kernel on the GPU, bit-exact), the engine
(prefill, decode, preemption, speculative decoding, grammar residency) and the HTTP fields."""

import json
import random
import re

import numpy as np
import pytest
import torch

from dstack_amd.ops import serving as sops
from dstack_amd.serving import guided
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.tokenizer import ByteTokenizer, HFTokenizer

# ------------------------------------------------------------------------------------------------
# 1. compiler against the stdlib
# ------------------------------------------------------------------------------------------------
# pattern -> matching strings the mutations start from; together: literals, ., classes, negated
# classes, \d \s \w and negations, groups, alternation, ? * + {m,n} (greedy and lazy), non-ASCII
REGEXES = {
    r"ab+c?": ["abbc", "ab"],
    r"(foo|ba[rz])*": ["foobarbaz", ""],
    r"\d{2,4}-\w+": ["123-ab_9", "00-x"],
    r"[^a-c]x.": ["dxé", "€xy"],
    r"é+|日本": ["éé", "日本"],
    r"\s*[A-Za-z_][\w]*\s*=\s*-?\d+(\.\d+)?": [" x_1 = -3.5", "a=1"],
    r"a{3}b{0,2}?": ["aaab", "aaa"],
    r"[\D]{1,2}": ["aé", "x"],
    r"(a|b)*abb": ["ababb", "abb"],
    r"\S\W": ["x!", "é€"],
    r"(?:x|yz)+?[0-9a-fA-F]*": ["xyzx0Af", "yz"],
    # prefix-closed languages: every live state accepts (the minimiser then starts from two blocks)
    r"(ab)*a?": ["ababa", "abab", ""],
    r"(yx)*y?": ["yxy", "yx"],
    r"[a-c]*": ["abcabc", "a"],
}


def _mutations(seeds, n, rng):
    for _ in range(n):
        s = bytearray(rng.choice(seeds).encode())
        for _ in range(rng.randint(0, 2)):
            k = rng.randint(0, 3)
            if k == 0 and s:
                del s[rng.randrange(len(s))]
            elif k == 1:
                s.insert(rng.randint(0, len(s)), rng.choice(b"abcx0 9-_=.\n\xc3\xa9\xe6!"))
            elif k == 2 and s:
                s[rng.randrange(len(s))] = rng.randrange(256)
            else:
                s += rng.choice(seeds).encode()
        yield bytes(s)


@pytest.mark.parametrize("pattern", list(REGEXES))
def test_regex_dfa_matches_re_fullmatch(pattern):
    """Acceptance of the DFA over bytes equals ``re.fullmatch`` (ASCII classes) on the decoded string;
    bytes that are no well-formed UTF-8 are never accepted.  Minimisation changes nothing."""
    rng = random.Random(sum(pattern.encode()))
    g, raw = guided.compile_regex(pattern), guided.compile_regex(pattern, minimise=False)
    assert g.states <= raw.states and not g.trans[0].any() and g.trans.dtype == np.uint16
    outcomes = set()
    for s in _mutations(REGEXES[pattern], 3000, rng):
        try:
            want = re.fullmatch(pattern, s.decode("utf-8"), re.ASCII) is not None
        except UnicodeDecodeError:
            want = False
        assert g.matches(s) == want, (pattern, s)
        assert raw.matches(s) == want, (pattern, s)
        outcomes.add(want)
    assert outcomes == {True, False}


def test_dfa_live_states_have_a_continuation_or_accept():
    g = guided.compile_regex(r"(ab|ac)d{0,2}")
    for s in range(1, g.states):
        assert g.accept[s] or g.trans[s].any()
    assert guided.advance(g, 1, b"ab") > 0 and guided.advance(g, 1, b"ad") == 0
    assert guided.compile_regex("a|b").key == guided.compile_regex("[ab]").key  # the hash is the DFA's


@pytest.mark.parametrize("pattern,names", [
    (r"(a)\1", "backreference"), (r"a(?=b)", "lookaround"), (r"a(?!b)", "lookaround"), (r"(?<=a)b", "lookaround"),
    (r"^a", "anchor"), (r"a$", "anchor"), (r"\bfoo", "anchor"), (r"(?i)abc", "flags"), (r"a(?i:b)", "flags"),
])
def test_unsupported_regex_constructs_raise_and_name_themselves(pattern, names):
    with pytest.raises(ValueError, match=names):
        guided.compile_regex(pattern)


def test_grammar_too_large():
    with pytest.raises(ValueError, match=r"grammar too large: 5002 states"):
        guided.compile_regex("[ab]{5000}")
    assert guided.compile_regex("[ab]{300}").states == 302
    assert guided.GUIDE_MAX_STATES == sops.GUIDE_MAX_STATES == 4096


def test_choice():
    g = guided.compile_choice(["a.b", "a+b", "日本"])
    assert all(g.matches(s.encode()) for s in ("a.b", "a+b", "日本"))
    assert not any(g.matches(s.encode()) for s in ("axb", "aab", "", "a.ba+b"))
    for bad in ([], ["x"] * 257, "abc", [1], [""]):
        with pytest.raises(ValueError, match="guided_choice"):
            guided.compile_choice(bad)


# ------------------------------------------------------------------------------------------------
# 2. schemas
# ------------------------------------------------------------------------------------------------
def _conforms(doc, schema, root=None):
    """A small checker of the supported subset: declaration order, no additional properties."""
    root = root or schema
    if "$ref" in schema:
        return _conforms(doc, root[schema["$ref"].split("/")[1]][schema["$ref"].split("/")[2]], root)
    for comb in ("anyOf", "oneOf"):
        if comb in schema:
            return any(_conforms(doc, s, root) for s in schema[comb])
    if "enum" in schema:
        return any(type(doc) is type(v) and doc == v for v in schema["enum"])
    if "const" in schema:
        return type(doc) is type(schema["const"]) and doc == schema["const"]
    types = schema["type"] if isinstance(schema["type"], list) else [schema["type"]]
    for t in types:
        if t == "null" and doc is None:
            return True
        if t == "boolean" and isinstance(doc, bool):
            return True
        if t == "integer" and isinstance(doc, int) and not isinstance(doc, bool):
            return True
        if t == "number" and isinstance(doc, (int, float)) and not isinstance(doc, bool):
            return True
        if t == "string" and isinstance(doc, str):
            if not schema.get("minLength", 0) <= len(doc) <= schema.get("maxLength", 10**9):
                continue
            if "pattern" in schema and not re.fullmatch(schema["pattern"], doc):
                continue
            return True
        if t == "array" and isinstance(doc, list):
            if not schema.get("minItems", 0) <= len(doc) <= schema.get("maxItems", 10**9):
                continue
            if all(_conforms(d, schema["items"], root) for d in doc):
                return True
        if t == "object" and isinstance(doc, dict):
            props, req = schema.get("properties", {}), schema.get("required", [])
            order = [k for k in props if k in doc]
            if list(doc) != order or any(r not in doc for r in req):
                continue
            if all(_conforms(doc[k], props[k], root) for k in doc):
                return True
    return False


PERSON = {
    "title": "Person", "type": "object", "additionalProperties": False,
    "properties": {
        "name": {"type": "string", "minLength": 1, "maxLength": 8, "description": "given name"},
        "age": {"type": ["integer", "null"]},
        "tags": {"type": "array", "items": {"enum": ["a", "b", 3]}, "minItems": 1, "maxItems": 3},
        "address": {"$ref": "#/$defs/address"},
        "score": {"anyOf": [{"type": "number"}, {"type": "boolean"}]},
    },
    "required": ["name", "tags"],
    "$defs": {"address": {"type": "object", "properties": {"zip": {"type": "string", "pattern": "[0-9]{5}"},
                                                           "city": {"const": "Paris"}}, "required": ["zip"]}},
}
ALL_OPTIONAL = {"type": "object", "properties": {"a": {"type": "boolean"}, "b": {"type": "null"},
                                                 "c": {"type": "array", "items": {"type": "integer"}, "maxItems": 2}}}
PERSON_DOCS = [
    {"name": "bob", "tags": ["a"]},
    {"name": "bob", "age": 3, "tags": ["a", 3], "address": {"zip": "75001", "city": "Paris"}, "score": 1.5},
    {"name": "é日", "age": None, "tags": ["b", "b", "b"], "score": True},
    {"name": "bob", "tags": []},  # minItems
    {"name": "bob", "tags": ["a", "a", "a", "a"]},  # maxItems
    {"name": "", "tags": ["a"]},  # minLength
    {"name": "bobbobbob", "tags": ["a"]},  # maxLength
    {"tags": ["a"], "name": "x"},  # declaration order
    {"name": "bob"},  # required
    {"name": "bob", "tags": ["c"]},  # enum
    {"name": "bob", "tags": ["a"], "extra": 1},  # additional property
    {"name": "bob", "tags": ["a"], "address": {"zip": "7500"}},  # pattern
    {"name": "bob", "tags": ["a"], "address": {"city": "Paris"}},  # required in $ref
    {"name": "bob", "tags": ["a"], "address": {"zip": "75001", "city": "Lyon"}},  # const
    {"name": "bob", "age": 1.5, "tags": ["a"]},  # integer
    {"name": "bob", "tags": ["a"], "score": "high"},  # anyOf
    {"name": 3, "tags": ["a"]},
]
OPTIONAL_DOCS = [{}, {"a": True}, {"b": None}, {"c": []}, {"a": False, "c": [1, -2]}, {"a": True, "b": None, "c": [0]},
                 {"b": None, "a": True}, {"c": [1, 2, 3]}, {"a": 1}, {"d": 1}, [], None]


@pytest.fixture(scope="module")
def person_guide():
    return guided.compile_json_schema(PERSON)


def test_schema_documents(person_guide):
    outcomes = set()
    for schema, g, docs in ((PERSON, person_guide, PERSON_DOCS),
                            (ALL_OPTIONAL, guided.compile_json_schema(ALL_OPTIONAL), OPTIONAL_DOCS)):
        for doc in docs:
            want = _conforms(doc, schema)
            for text in (json.dumps(doc), json.dumps(doc, separators=(",", ":")), json.dumps(doc, ensure_ascii=False)):
                assert g.matches(text.encode()) == want, (text, want)
            outcomes.add(want)
    assert outcomes == {True, False}
    # hand-written: at most one space at a structural gap, no newlines
    assert person_guide.matches(b'{ "name": "x", "tags": [ "a" ] }')
    assert not person_guide.matches(b'{"name":  "x","tags":["a"]}')
    assert not person_guide.matches(b'{"name":"x",\n"tags":["a"]}')
    assert not person_guide.matches(b'{"name":"x","tags":["a"]')


def _random_doc(rng, depth):
    """A random JSON value whose containers nest exactly ``depth`` deep on one path."""
    scalars = [None, True, False, 0, -12, 3.25, 1e-7, "", "text", 'q"\\\n\t', "é日本"]
    if depth == 0:
        return rng.choice(scalars)
    inner = [_random_doc(rng, depth - 1)] + [_random_doc(rng, rng.randint(0, depth - 1)) for _ in range(rng.randint(0, 2))]
    rng.shuffle(inner)
    if rng.random() < 0.5:
        return inner
    return {f"k{i}": v for i, v in enumerate(inner)}


@pytest.fixture(scope="module")
def json_object_guide():
    return guided.compile_json_object()


def test_json_object(json_object_guide):
    g, rng = json_object_guide, random.Random(5)
    assert g.states <= guided.GUIDE_MAX_STATES and guided.JSON_OBJECT_DEPTH == 4
    for _ in range(150):
        depth = rng.randint(0, 5)
        doc = {"top": _random_doc(rng, depth), "more": _random_doc(rng, rng.randint(0, depth))}  # values `depth` deep
        for text in (json.dumps(doc), json.dumps(doc, separators=(",", ":")), json.dumps(doc, ensure_ascii=False)):
            assert g.matches(text.encode()) == (depth <= 4), (depth, text)
            assert not g.matches(text.encode()[:-1])  # truncated
            assert not g.matches(text.encode()[: len(text) // 2])
    assert g.matches(b"{}") and g.matches(b"{ }") and not g.matches(b"{  }")
    for text in ("[1]", "[]", "1", '"x"', "null", '{"a":1}{"b":2}', '{"a":1,}', "{'a':1}", '{"a":01}', '{"a":"\x01"}'):
        assert not g.matches(text.encode()), text


@pytest.mark.parametrize("schema,name", [
    ({"type": "string", "format": "date"}, "format"),
    ({"type": "integer", "minimum": 1}, "minimum"),
    ({"type": "object", "patternProperties": {}}, "patternProperties"),
    ({"type": "object", "additionalProperties": True}, "additionalProperties"),
    ({"type": "object", "additionalProperties": {"type": "string"}}, "additionalProperties"),
    ({"not": {"type": "null"}}, "not"),
    ({"type": "array", "items": {"type": "null"}, "uniqueItems": True}, "uniqueItems"),
    ({"allOf": [{"type": "null"}]}, "allOf"),
    ({"type": "tuple"}, "tuple"),
    ({"$ref": "#/$defs/a", "$defs": {"a": {"type": "array", "items": {"$ref": "#/$defs/a"}}}}, r"recursive \$ref"),
    ({"$ref": "http://example.com/schema"}, r"\$ref"),
    ({"type": "string", "pattern": "(a)\\1"}, "backreference"),
    # a pattern that could put a quote, a backslash or a control character between the quotes
    ({"type": "string", "pattern": ".*"}, "pattern"),
    ({"type": "string", "pattern": "[^x]+"}, "pattern"),
    ({"type": "string", "pattern": "a\\\\b"}, "pattern"),
    ({"type": "string", "pattern": "\\s+"}, "pattern"),
])
def test_refused_schema_keywords_are_named(schema, name):
    with pytest.raises(ValueError, match=name):
        guided.compile_json_schema(schema)


# ------------------------------------------------------------------------------------------------
# 3. token bytes
# ------------------------------------------------------------------------------------------------
def test_byte_tokenizer_token_bytes():
    tok = ByteTokenizer(1024)
    table = tok.token_bytes()
    assert len(table) == 1024 and table[:3] == [b"", b"", b""] and table[3 + 65] == b"A" and table[3 + 256 + 65] == b"A"
    rng = random.Random(0)
    for _ in range(50):
        ids = [rng.randrange(1024) for _ in range(rng.randint(0, 40))]
        assert b"".join(table[i] for i in ids).decode("utf-8", errors="replace") == tok.decode(ids)


CORPUS = ["the quick brown fox jumps over the lazy dog", "héllo wörld, naïve café", "日本語のテキスト と 漢字",
          '{"name": "bob", "tags": [1, 2, 3]}', "    indented\n\tcode(x) -> y"] * 4


def _save(tok, tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    tok.save(str(d / "tokenizer.json"))
    return HFTokenizer(str(d))


def test_hf_bytelevel_token_bytes(tmp_path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers

    t = Tokenizer(models.BPE())
    t.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    t.decoder = decoders.ByteLevel()
    t.train_from_iterator(CORPUS, trainers.BpeTrainer(vocab_size=420, show_progress=False, special_tokens=["<|eot_id|>"],
                                                      initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    tok = _save(t, tmp_path, "bytelevel")
    table = tok.token_bytes()
    assert len(table) == tok.vocab_size and table[t.token_to_id("<|eot_id|>")] == b""
    assert sorted(b for b in table if len(b) == 1) == [bytes([i]) for i in range(256)]  # the whole byte alphabet
    assert any(len(b) > 2 for b in table)
    rng = random.Random(1)
    for text in CORPUS[:5]:
        ids = tok.encode(text, add_bos=False)
        assert b"".join(table[i] for i in ids) == text.encode()
    for _ in range(200):
        ids = [rng.randrange(len(table)) for _ in range(rng.randint(1, 12))]
        assert b"".join(table[i] for i in ids).decode("utf-8", errors="replace") == tok.decode(ids), ids


def test_hf_metaspace_bytefallback_token_bytes(tmp_path):
    from tokenizers import Tokenizer, decoders, models

    pieces = ["<unk>"] + [f"<0x{b:02X}>" for b in range(256)] + ["▁", "▁the", "he", "llo", "▁wor", "ld", "é", "日本", "a", "▁▁"]
    t = Tokenizer(models.BPE(vocab={p: i for i, p in enumerate(pieces)}, merges=[], unk_token="<unk>", byte_fallback=True))
    t.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse(),
                                   decoders.Strip(" ", 1, 0)])
    tok = _save(t, tmp_path, "metaspace")
    table = tok.token_bytes()
    assert table[1 + 0x41] == b"A" and table[pieces.index("▁the")] == b" the" and table[pieces.index("日本")] == "日本".encode()
    rng = random.Random(2)
    for _ in range(200):
        ids = []
        for _ in range(rng.randint(1, 10)):
            if rng.random() < 0.4:  # a character spelled in byte tokens
                ids += [1 + b for b in rng.choice("xé€日😀\n").encode()]
            else:
                ids.append(rng.randrange(257, len(pieces)))
        mine = b"".join(table[i] for i in ids).decode("utf-8", errors="replace")
        theirs = tok.decode(ids)
        assert theirs == (mine[1:] if mine.startswith(" ") else mine), ids  # the decoder strips one leading space
    # random ids, byte tokens included -- the ASCII ones: the library turns a whole run of byte tokens
    # that is no UTF-8 into replacement characters, valid bytes inside it included, where a decoder of
    # the concatenated bytes replaces only the invalid ones (a grammar never lets such a run through)
    ascii_ids = list(range(1, 1 + 128)) + list(range(257, len(pieces)))
    for _ in range(200):
        ids = [rng.choice(ascii_ids) for _ in range(rng.randint(1, 10))]
        mine = b"".join(table[i] for i in ids).decode("utf-8", errors="replace")
        assert tok.decode(ids) == (mine[1:] if mine.startswith(" ") else mine), ids


def test_other_tokenizers_refuse_token_bytes(tmp_path):
    from tokenizers import Tokenizer, models, pre_tokenizers

    t = Tokenizer(models.WordLevel({"[UNK]": 0, "the": 1}, unk_token="[UNK]"))
    t.pre_tokenizer = pre_tokenizers.Whitespace()
    with pytest.raises(ValueError, match="ByteLevel or Metaspace"):
        _save(t, tmp_path, "wordlevel").token_bytes()


# ------------------------------------------------------------------------------------------------
# 4. reference mask
# ------------------------------------------------------------------------------------------------
def _pool(guides, device="cpu"):
    """trans int16 [G, 4096, 256] / accept uint8 [G, 4096] holding ``guides`` ((trans, accept) arrays)."""
    trans = torch.zeros(len(guides), sops.GUIDE_MAX_STATES, 256, dtype=torch.int16)
    accept = torch.zeros(len(guides), sops.GUIDE_MAX_STATES, dtype=torch.uint8)
    for i, (t, a) in enumerate(guides):
        trans[i, : len(t)] = torch.from_numpy(np.asarray(t, dtype=np.uint16).view(np.int16))
        accept[i, : len(a)] = torch.from_numpy(np.asarray(a, dtype=np.uint8))
    return trans.to(device), accept.to(device)


def _table(tokens, vocab, device="cpu"):
    off, blob = guided.pack_token_bytes(tokens, vocab)
    return torch.from_numpy(off).to(device), torch.from_numpy(blob).to(device)


def _ab_star():
    """a b*: 0 dead, 1 start, 2 accepting."""
    t = np.zeros((3, 256), dtype=np.uint16)
    t[1, ord("a")] = 2
    t[2, ord("b")] = 2
    return t, np.array([0, 0, 1], dtype=np.uint8)


def test_apply_guide_ref_kept_sets():
    tokens = [b"", b"", b"a", b"b", b"ab", b"abb", b"ba", b"abc", b"c", b"bb", b"aa", b"bbbc"]  # 1: EOS
    trans, accept = _pool([_ab_star()])
    off, blob = _table(tokens, 12)
    eos, n_eos = torch.tensor([1, -1], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    logits = torch.randn(3, 12).to(torch.bfloat16)
    guide = torch.tensor([0, 0, -1], dtype=torch.int32)
    state = torch.tensor([1, 2, 1], dtype=torch.int32)
    out = sops.apply_guide_ref(logits, guide, state, trans, accept, off, blob, eos, n_eos)
    kept = [set(torch.nonzero(~torch.isneginf(out[r].float())).flatten().tolist()) for r in range(3)]
    assert kept[0] == {2, 4, 5}  # a, ab, abb; "abc" dies on its last byte; no EOS outside an accepting state
    assert kept[1] == {1, 3, 9}  # EOS, b, bb; "bbbc" dies on its last byte; the empty token 0 never
    for r in range(2):
        k = sorted(kept[r])
        assert torch.equal(out[r, k].view(torch.int16), logits[r, k].view(torch.int16))
    assert torch.equal(out[2].view(torch.int16), logits[2].view(torch.int16))
    # the in-place CPU path writes the same and leaves the -1 row alone
    x = logits.clone()
    assert sops.apply_guide(x, guide, state, trans, accept, off, blob, eos, n_eos) is x
    assert torch.equal(x.view(torch.int16), out.view(torch.int16))
    # out-of-range guide / state: untouched
    bad = sops.apply_guide_ref(logits, torch.tensor([1, 0, -7], dtype=torch.int32),
                               torch.tensor([1, 4096, 1], dtype=torch.int32), trans, accept, off, blob, eos, n_eos)
    assert torch.equal(bad.view(torch.int16), logits.view(torch.int16))


# ------------------------------------------------------------------------------------------------
# 5. engine end to end (tiny random-weight model, ByteTokenizer, CPU)
# ------------------------------------------------------------------------------------------------
TOK = ByteTokenizer(1024)
EOS = ByteTokenizer.EOS
# bounded grammars: every path ends, so even a greedy random model reaches a state where only EOS is left
REGEX = r"(yes|no|maybe)-[0-9]{3}-[a-f]{1,4}"
CHOICES = ["alpha", "beta", "gamma delta"]
ROBOT = {"type": "object", "required": ["name", "on"], "properties": {
    "name": {"type": "string", "minLength": 1, "maxLength": 6}, "on": {"type": "boolean"},
    "mode": {"enum": ["idle", "run", 7, None]},
    "pos": {"type": "array", "items": {"enum": [0, 1, -1]}, "minItems": 2, "maxItems": 3}}}
SAMPLING = [(0.0, None), (1.5, 11), (1.5, 12)]  # (temperature, seed)
# a greedy random model either closes a json_object at once or loops inside a string up to max_tokens
# (a legitimate "length"); after this prompt it closes.  The seeded rows walk the deep paths.
PROMPT = "Reply in JSON: "


def _engine(device="cpu", **kw):
    args = dict(device=device, max_model_len=2048, max_batch=8, num_pages=64)
    args.update(kw)
    eng = LLMEngine.from_model("llama-tiny", **args)
    eng.eos_token_ids = (EOS,)
    return eng


def _text(req):
    assert req.output_ids[-1] == EOS
    return TOK.decode(req.output_ids[:-1])


def _robot_ok(text):
    try:
        return _conforms(json.loads(text), ROBOT)
    except ValueError:
        return False


def _object_ok(text):
    try:
        return isinstance(json.loads(text), dict)
    except ValueError:
        return False


@pytest.fixture(scope="module")
def guides(json_object_guide):
    return {"regex": (guided.compile_regex(REGEX), lambda s: re.fullmatch(REGEX, s) is not None),
            "choice": (guided.compile_choice(CHOICES), lambda s: s in CHOICES),
            "schema": (guided.compile_json_schema(ROBOT), _robot_ok),
            "json_object": (json_object_guide, _object_ok)}


@pytest.fixture(scope="module")
def cpu_engine():
    return _engine()


def _run_kinds(eng, guides, kinds, max_tokens=1500):
    prompt = TOK.encode(PROMPT)
    params, checks = [], []
    for kind in kinds:
        g, ok = guides[kind]
        for temp, seed in SAMPLING:
            params.append(SamplingParams(max_tokens=max_tokens, temperature=temp, seed=seed, guide=g))
            checks.append((kind, ok))
    reqs = eng.generate([prompt] * len(params), params)
    for r, (kind, ok) in zip(reqs, checks):
        assert r.finish_reason == "stop", (kind, r.params.temperature, r.params.seed, len(r.output_ids))
        assert ok(_text(r)), (kind, _text(r))
    return reqs


def test_engine_guided_outputs_conform(cpu_engine, guides):
    reqs = _run_kinds(cpu_engine, guides, ["regex", "choice", "schema", "json_object"])
    assert len({tuple(r.output_ids) for r in reqs}) > 6  # seeds and grammars give different outputs
    # the same prompts, seeds and temperatures unguided: nothing conforms, so the above is not vacuous
    plain = cpu_engine.generate([TOK.encode(PROMPT)] * len(reqs),
                                [SamplingParams(max_tokens=40, temperature=r.params.temperature, seed=r.params.seed)
                                 for r in reqs])
    for r in plain:
        text = TOK.decode(r.output_ids)
        assert not any(ok(text) for _, ok in guides.values()), text
    assert not cpu_engine._guide_refs and cpu_engine.metrics()["guided_grammars_resident"] >= 4


def test_engine_mixed_batch_leaves_unguided_rows_alone(cpu_engine, guides):
    prompts = [TOK.encode(p) for p in ("one", "two two", "three", "four 4")]
    base = [SamplingParams(max_tokens=40, temperature=t, seed=s) for t, s in ((1.0, 1), (0.0, None), (1.0, 3), (0.8, 4))]
    mixed = [SamplingParams(max_tokens=40, temperature=1.0, seed=1, guide=guides["regex"][0]), base[1],
             SamplingParams(max_tokens=40, temperature=1.0, seed=3, guide=guides["schema"][0]), base[3]]
    a = cpu_engine.generate(prompts, mixed)
    b = cpu_engine.generate(prompts, base)
    assert a[1].output_ids == b[1].output_ids and a[3].output_ids == b[3].output_ids
    assert re.fullmatch(REGEX, _text(a[0])) and _robot_ok(_text(a[2]))
    assert a[0].output_ids != b[0].output_ids


def test_engine_guided_request_survives_preemption(guides):
    prompts = [[1 + i, 2, 3, 4 + i] * (5 + i) for i in range(4)]
    rx = guided.compile_regex(r"[a-z]{70}")  # long enough to be preempted on the way
    params = [SamplingParams(max_tokens=80, temperature=1.0, seed=20 + i, guide=rx if i % 2 == 0 else None,
                             ignore_eos=i % 2 == 1) for i in range(4)]
    kw = dict(max_model_len=256)
    big = _engine(num_pages=64, **kw).generate(prompts, params)
    small_eng = _engine(num_pages=5, **kw)
    small = small_eng.generate(prompts, params)
    assert small_eng.stats["preemptions"] > 0
    assert [r.output_ids for r in small] == [r.output_ids for r in big]
    for r in (small[0], small[2]):
        assert r.finish_reason == "stop" and re.fullmatch(r"[a-z]{70}", _text(r))


def test_engine_speculative_decoding_keeps_guided_outputs(cpu_engine, guides):
    spec = _engine(speculative_ngram=3)
    literal = "The quick brown fox jumps over the lazy dog."
    forced = guided.compile_regex(re.escape(literal) + "[0-9]{2}")
    prompt = TOK.encode("Repeat after me: " + literal + " Again: ")
    params = [SamplingParams(max_tokens=200, temperature=t, seed=s, guide=g)
              for g in (forced, guides["schema"][0], guides["regex"][0]) for t, s in ((0.0, None), (1.5, 5))]
    want = cpu_engine.generate([prompt] * len(params), params)
    got = spec.generate([prompt] * len(params), params)
    assert [r.output_ids for r in got] == [r.output_ids for r in want]
    assert all(r.finish_reason == "stop" for r in got) and _text(got[0]).startswith(literal)
    assert spec.stats["spec_accepted"] > 0 and spec.stats["spec_drafted"] >= spec.stats["spec_accepted"]


def test_engine_one_slot_two_grammars(guides):
    eng = _engine(max_guides=1)
    prompt = TOK.encode(PROMPT)
    a = eng.add_request(prompt, SamplingParams(max_tokens=100, temperature=1.0, seed=1, guide=guides["regex"][0]))
    b = eng.add_request(prompt, SamplingParams(max_tokens=100, temperature=1.0, seed=2, guide=guides["choice"][0]))
    eng.step()
    assert len(a.output_ids) == 1 and not b.output_ids and eng._pending == [b]  # b waits for the only slot
    while not (a.finished and b.finished):
        assert a.finished or not b.output_ids
        eng.step()
    assert a.finish_reason == b.finish_reason == "stop"
    assert re.fullmatch(REGEX, _text(a)) and _text(b) in CHOICES
    assert eng.metrics()["guided_grammars_resident"] == 1 and eng.stats["guided_requests"] == 2


def test_engine_refusals(guides):
    g = guides["choice"][0]
    with pytest.raises(ValueError, match="max_guides"):
        _engine(max_guides=0).add_request([5, 6], SamplingParams(guide=g))
    eng = _engine(max_guides=2)
    with pytest.raises(ValueError, match="ignore_eos"):
        eng.add_request([5, 6], SamplingParams(guide=g, ignore_eos=True))
    with pytest.raises(ValueError, match="compiled grammar"):
        eng.add_request([5, 6], SamplingParams(guide="a|b"))
    with pytest.raises(ValueError, match="max_guides"):
        _engine(max_guides=-1)
    assert not hasattr(_engine(max_guides=0), "g_trans")


def test_engine_logit_bias_cannot_force_an_illegal_token(cpu_engine, guides):
    illegal = TOK.encode("z", add_bos=False)[0]  # no choice holds a z
    sp = SamplingParams(max_tokens=30, temperature=0.0, guide=guides["choice"][0], logit_bias={illegal: 100})
    free = cpu_engine.generate([TOK.encode(PROMPT)], SamplingParams(max_tokens=5, temperature=0.0, ignore_eos=True,
                                                                    logit_bias={illegal: 100}))[0]
    assert free.output_ids == [illegal] * 5  # the bias does force it where nothing forbids it
    r = cpu_engine.generate([TOK.encode(PROMPT)], sp)[0]
    assert illegal not in r.output_ids and r.finish_reason == "stop" and _text(r) in CHOICES


def test_engine_host_walk_catches_a_mask_that_lets_everything_through(monkeypatch, guides):
    """The host is the source of truth: with the mask switched off, a forced illegal token and a forced
    EOS outside an accepting state are raised as engine bugs, not emitted."""
    monkeypatch.setattr(sops, "apply_guide", lambda logits, *a, **k: logits)
    illegal = TOK.encode("z", add_bos=False)[0]
    for forced, message in ((illegal, "refuses"), (EOS, "EOS")):
        eng = _engine()
        eng.add_request(TOK.encode(PROMPT), SamplingParams(max_tokens=5, temperature=0.0, guide=guides["choice"][0],
                                                           logit_bias={forced: 100}))
        with pytest.raises(RuntimeError, match=message):
            eng.step()


# ------------------------------------------------------------------------------------------------
# 6. server
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    eng = LLMEngine.from_model("llama-tiny", device="cpu", max_model_len=1024, max_batch=8, num_pages=64)
    app = create_app(eng, served_model_name="llama-tiny")
    with TestClient(app) as c:
        yield c


def _fields():
    return {"guided_regex": (REGEX, lambda s: re.fullmatch(REGEX, s) is not None),
            "guided_choice": (CHOICES, lambda s: s in CHOICES),
            "guided_json": (ROBOT, _robot_ok),
            "response_format": ({"type": "json_schema", "json_schema": {"name": "robot", "schema": ROBOT}}, _robot_ok)}


@pytest.mark.parametrize("field", list(_fields()))
def test_api_fields_on_both_routes(api, field):
    value, ok = _fields()[field]
    common = {"model": "llama-tiny", "max_tokens": 200, "temperature": 1.2, "seed": 3, field: value}
    r = api.post("/v1/completions", json=dict(common, prompt=PROMPT))
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert ch["finish_reason"] == "stop" and ok(ch["text"]), ch
    r = api.post("/v1/chat/completions", json=dict(common, messages=[{"role": "user", "content": "hi"}]))
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert ch["finish_reason"] == "stop" and ok(ch["message"]["content"]), ch
    for route, extra in (("/v1/completions", {"prompt": PROMPT}),
                         ("/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}]})):
        with api.stream("POST", route, json=dict(common, stream=True, **extra)) as r:
            assert r.status_code == 200
            lines = [ln for ln in r.iter_lines() if ln.startswith("data: ")]
        chunks = [json.loads(ln[6:])["choices"][0] for ln in lines[:-1]]
        text = "".join(c["text"] if "text" in c else c["delta"].get("content", "") for c in chunks)
        assert chunks[-1]["finish_reason"] == "stop" and ok(text), text


def test_schema_string_pattern_stays_json():
    g = guided.compile_json_schema({"type": "string", "pattern": r"^[^\"\\\x00-\x1f]{0,3}$"})
    for s in ("", "ab", "é日x"):
        assert g.matches(json.dumps(s, ensure_ascii=False).encode())
    assert not g.matches(b'"a"b"') and not g.matches(b'"a\\"') and not g.matches(b'"abcd"') and not g.matches(b'"\n"')


def test_api_json_object_on_both_routes_and_streamed(api):
    common = {"model": "llama-tiny", "max_tokens": 900, "temperature": 1.5, "seed": 11,
              "response_format": {"type": "json_object"}}
    chat = {"messages": [{"role": "user", "content": "hi"}]}
    ch = api.post("/v1/chat/completions", json=dict(common, **chat)).json()["choices"][0]
    assert ch["finish_reason"] == "stop" and _object_ok(ch["message"]["content"]), ch
    for route, extra in (("/v1/completions", {"prompt": PROMPT}), ("/v1/chat/completions", chat)):
        with api.stream("POST", route, json=dict(common, stream=True, **extra)) as r:
            assert r.status_code == 200
            lines = [ln for ln in r.iter_lines() if ln.startswith("data: ")]
        chunks = [json.loads(ln[6:])["choices"][0] for ln in lines[:-1]]
        text = "".join(c["text"] if "text" in c else c["delta"].get("content", "") for c in chunks)
        assert chunks[-1]["finish_reason"] == "stop" and _object_ok(text), text


def test_api_json_object_and_text(api):
    body = {"model": "llama-tiny", "prompt": PROMPT, "max_tokens": 900, "temperature": 1.5, "seed": 11,
            "response_format": {"type": "json_object"}}
    ch = api.post("/v1/completions", json=body).json()["choices"][0]
    assert ch["finish_reason"] == "stop" and _object_ok(ch["text"]), ch
    # text asks for nothing, also next to a guided_* field
    r = api.post("/v1/completions", json=dict(body, response_format={"type": "text"}, max_tokens=4))
    assert r.status_code == 200 and r.json()["choices"][0]["finish_reason"] == "length"
    r = api.post("/v1/completions", json=dict(body, response_format={"type": "text"}, guided_choice=CHOICES))
    assert r.status_code == 200 and r.json()["choices"][0]["text"] in CHOICES


@pytest.mark.parametrize("extra,names", [
    ({"guided_regex": "a+", "guided_choice": ["a"]}, ["guided_regex", "guided_choice"]),  # two fields at once
    ({"response_format": {"type": "json_object"}, "guided_json": ROBOT}, ["response_format", "guided_json"]),
    ({"guided_json": {"type": "object", "properties": 3}}, ["guided_json"]),  # a bad schema
    ({"guided_json": "{not json"}, ["guided_json"]),
    ({"response_format": {"type": "json_schema", "json_schema": {"name": "x"}}}, ["response_format"]),
    ({"response_format": {"type": "yaml"}}, ["response_format"]),
    ({"guided_json": {"type": "string", "format": "email"}}, ["guided_json", "format"]),  # an unsupported keyword
    ({"guided_regex": "a(?=b)"}, ["guided_regex", "lookaround"]),
    ({"guided_regex": "[ab]{5000}"}, ["guided_regex", "grammar too large"]),  # an oversized grammar
    ({"guided_choice": []}, ["guided_choice"]),
    ({"guided_choice": ["a"], "ignore_eos": True}, ["ignore_eos", "guided_choice"]),
])
def test_api_refusals_name_the_field(api, extra, names):
    for route, body in (("/v1/completions", {"prompt": "x"}), ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}]})):
        r = api.post(route, json=dict(body, model="llama-tiny", max_tokens=5, **extra))
        assert r.status_code == 400, r.text
        msg = r.json()["error"]["message"]
        assert all(n in msg for n in names), msg


def test_api_metrics_count_guided_requests(api):
    def metric(name):
        line = next(ln for ln in api.get("/metrics").text.splitlines() if ln.startswith(name + " "))
        return float(line.split()[1])

    n0, c0 = metric("dstack_serving_guided_requests_total"), metric("dstack_serving_guided_compile_seconds_total")
    body = {"model": "llama-tiny", "prompt": "x", "max_tokens": 20, "guided_regex": "metrics-[0-9]"}
    for _ in range(2):
        assert api.post("/v1/completions", json=body).status_code == 200
    assert metric("dstack_serving_guided_requests_total") == n0 + 2
    c1 = metric("dstack_serving_guided_compile_seconds_total")
    assert c1 > c0  # compiled once ...
    assert api.post("/v1/completions", json=body).status_code == 200
    assert metric("dstack_serving_guided_compile_seconds_total") == c1  # ... then served from the cache
    assert metric("dstack_serving_guided_grammars_resident") >= 1


# ------------------------------------------------------------------------------------------------
# GPU: the HIP kernel against the reference (bit-exact), in a captured graph, in the engine
# ------------------------------------------------------------------------------------------------
def _two_grammars():
    """0: (ab|abc)?d* -- start accepting with continuations; 1: xy{2} -- ends in an accepting state with none."""
    return guided.compile_regex(r"(ab|abc)?d*"), guided.compile_regex(r"xy{2}")


def _gpu_tokens(V, ntok, rng):
    long = b"abc" + b"d" * 37  # 40 bytes, legal from the start of grammar 0
    assert len(long) == 40
    tokens = [b"", b"", b"", b"a", b"b", b"c", b"d", b"x", b"y", b"ab", b"abc", b"abd", b"dd", b"xy", b"xyy", b"yy",
              b"xyyy", long, long[:-1] + b"x", b"abcd", b"abab"]
    alphabet = b"abcdxy"
    while len(tokens) < ntok:
        n = rng.choice([0, 1, 1, 2, 3, 5])
        tokens.append(bytes(rng.choice(alphabet) for _ in range(n)))
    return tokens


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1000, 4107])  # one partial span; two spans with a tail that is no multiple of 8
@pytest.mark.parametrize("pad", [0, 1])  # row stride V (rows 16-byte aligned when V % 8 == 0) and V + 1 (unaligned)
def test_gpu_apply_guide_matches_reference(gpu, V, pad):
    rng = random.Random(V + pad)
    g0, g1 = _two_grammars()
    ntok = V - 37  # ids from ntok on are beyond the tokenizer's size: empty
    tokens = _gpu_tokens(V, ntok, rng)
    trans, accept = _pool([(g0.trans, g0.accept), (g1.trans, g1.accept)], gpu)
    off, blob = _table(tokens, ntok, gpu)
    assert off.numel() == ntok + 1
    eos = torch.tensor([1, 2, -1, -1], dtype=torch.int32, device=gpu)  # two EOS ids
    n_eos = torch.tensor([2], dtype=torch.int32, device=gpu)
    mid0, end1 = guided.walk(g0, 1, b"a"), guided.walk(g1, 1, b"xyy")
    assert mid0 and not g0.accept[mid0] and g0.accept[1] and g0.trans[1].any()  # mid-literal; accepting with continuations
    assert g1.accept[end1] and not g1.trans[end1].any() and not g1.accept[1]  # accepting with none; plain start
    torch.manual_seed(V)
    base = (torch.randn(3, V + pad) * 4).to(torch.bfloat16)
    base[:, 5] = float("-inf")
    base[:, 6] = float("inf")
    base[:, 17] = float("inf")
    base[:, V - 1] = float("-inf")
    cases = [([0, -1, 1], [1, 1, 1]),  # both start states
             ([0, -1, 1], [mid0, 7, end1]),
             ([1, -1, 0], [guided.walk(g1, 1, b"x"), 0, guided.walk(g0, 1, b"abc")]),
             ([0, 1, 0], [0, 1, 1]),  # the dead state: everything goes
             ([2, -1, 1], [1, 1, 4096]), ([-5, 0, 1], [1, -1, 1 << 20])]  # out-of-range guide / state: untouched
    for guide, state in cases:
        x = base.to(gpu)[:, :V]
        assert x.stride(0) == V + pad
        gt = torch.tensor(guide, dtype=torch.int32, device=gpu)
        st = torch.tensor(state, dtype=torch.int32, device=gpu)
        want = sops.apply_guide_ref(base[:, :V], gt.cpu(), st.cpu(), trans.cpu(), accept.cpu(), off.cpu(), blob.cpu(),
                                    eos.cpu(), n_eos.cpu())
        assert sops.apply_guide(x, gt, st, trans, accept, off, blob, eos, n_eos) is x
        assert torch.equal(x.cpu().view(torch.int16), want.view(torch.int16)), (guide, state)
        for r, (gi, si) in enumerate(zip(guide, state)):
            if not (0 <= gi < 2 and 0 <= si < 4096):
                assert torch.equal(x[r].cpu().view(torch.int16), base[r, :V].view(torch.int16))
        if pad:  # the column past the row is not the kernel's
            assert torch.equal(x.as_strided((3,), (V + pad,), V).cpu().view(torch.int16), base[:, V].view(torch.int16))
    # the reference itself keeps what it should in the first case (not everything, not nothing)
    want = sops.apply_guide_ref(base[:, :V], torch.tensor([0, -1, 1], dtype=torch.int32), torch.tensor([1, 1, 1], dtype=torch.int32),
                                trans.cpu(), accept.cpu(), off.cpu(), blob.cpu(), eos.cpu(), n_eos.cpu())
    kept = ~torch.isneginf(want[0].float())
    assert kept[17] and kept[1] and kept[2] and not kept[0] and not kept[18] and not kept[7] and not kept[V - 1]
    assert 10 < int(kept.sum()) < V // 2


@pytest.mark.gpu
def test_gpu_apply_guide_in_a_captured_graph(gpu):
    V, rows = 1000, 4
    rng = random.Random(3)
    g0, g1 = _two_grammars()
    tokens = _gpu_tokens(V, V, rng)
    trans, accept = _pool([(g0.trans, g0.accept), (g1.trans, g1.accept)], gpu)
    off, blob = _table(tokens, V, gpu)
    eos = torch.tensor([1, 2], dtype=torch.int32, device=gpu)
    n_eos = torch.tensor([2], dtype=torch.int32, device=gpu)
    torch.manual_seed(0)
    src = (torch.randn(rows, V, device=gpu) * 3).to(torch.bfloat16)
    logits = torch.empty_like(src)
    guide = torch.tensor([0, 1, -1, 0], dtype=torch.int32, device=gpu)
    state = torch.ones(rows, dtype=torch.int32, device=gpu)
    temps = torch.full((rows,), 1.0, device=gpu)
    seeds = torch.arange(rows, dtype=torch.int64, device=gpu)
    steps = torch.zeros(rows, dtype=torch.int32, device=gpu)
    top_k = torch.zeros(rows, dtype=torch.int32, device=gpu)
    top_p, min_p = torch.ones(rows, device=gpu), torch.zeros(rows, device=gpu)
    out_tok = torch.zeros(rows, dtype=torch.int32, device=gpu)
    out_lp, tau = torch.zeros(rows, device=gpu), torch.zeros(rows, device=gpu)

    def body():
        logits.copy_(src)
        sops.apply_guide(logits, guide, state, trans, accept, off, blob, eos, n_eos)
        sops.sample_filtered(logits, temps, seeds, steps, top_k, top_p, min_p, out_tok, out_lp, tau=tau)

    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    staged = [[1, 1, 1, 1], [guided.walk(g0, 1, b"a"), guided.walk(g1, 1, b"x"), 9, guided.walk(g0, 1, b"abc")],
              [guided.walk(g0, 1, b"abd"), guided.walk(g1, 1, b"xyy"), 0, guided.walk(g0, 1, b"ab")]]
    seen = []
    for st in staged:
        state.copy_(torch.tensor(st, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize(gpu)
        want = sops.apply_guide_ref(src.cpu(), guide.cpu(), state.cpu(), trans.cpu(), accept.cpu(), off.cpu(), blob.cpu(),
                                    eos.cpu(), n_eos.cpu())
        toks = out_tok.tolist()
        for r in range(rows):
            assert not torch.isneginf(want[r, toks[r]].float()), (st, r, toks[r])
        assert torch.equal(logits.cpu().view(torch.int16), want.view(torch.int16))
        seen.append(toks)
    assert seen[0][2] == seen[1][2] == seen[2][2]  # the unguided row: same draw every time
    assert len({tuple(t) for t in seen}) == 3  # the guided rows follow the staged state
    assert seen[2][1] in (1, 2)  # grammar 1 after "xyy": only EOS is left


@pytest.mark.gpu
def test_gpu_engine_guided_with_captured_graphs(gpu, guides):
    eng = _engine(device="cuda", max_model_len=512)
    eng.capture_graphs()
    assert eng._graphs
    _run_kinds(eng, guides, ["regex", "schema"], max_tokens=200)
    # guided and unguided rows in one bucket: the unguided rows' tokens do not depend on the guides
    prompts = [TOK.encode(p) for p in ("one", "two two", "three", "four 4")]
    base = [SamplingParams(max_tokens=60, temperature=t, seed=s, ignore_eos=True) for t, s in ((1.0, 1), (0.0, None), (1.0, 3), (0.8, 4))]
    filler = guided.compile_regex(r"[a-z ]{70}")  # as long as the unguided rows run: the bucket stays the same
    mixed = [SamplingParams(max_tokens=60, temperature=1.0, seed=1, guide=filler), base[1],
             SamplingParams(max_tokens=60, temperature=1.0, seed=3, guide=filler), base[3]]
    plain = [SamplingParams(max_tokens=60, temperature=1.0, seed=1, ignore_eos=True), base[1],
             SamplingParams(max_tokens=60, temperature=1.0, seed=3, ignore_eos=True), base[3]]
    a = eng.generate(prompts, mixed)
    b = eng.generate(prompts, plain)
    assert a[1].output_ids == b[1].output_ids and a[3].output_ids == b[3].output_ids
    assert re.fullmatch(r"[a-z ]{60}", TOK.decode(a[0].output_ids)) and a[0].output_ids != b[0].output_ids
