"""Structured outputs: regular expressions, choices and JSON schemas compiled to byte-level DFAs.

Every constraint becomes a regular expression and then a deterministic automaton over UTF-8 bytes:
regex -> NFA (Thompson) -> DFA (subset construction) -> pruned and minimised DFA.  The engine keeps the
automaton's state per request (one integer) and ``ops.serving.apply_guide`` masks, inside the decode
graph, every token whose bytes the automaton refuses.  Pure Python + numpy, on the CPU, at request
time (the HTTP server compiles in the request handler and caches; never on the engine loop).

DFA encoding (``Guide``): state 0 is dead (all its transitions go to 0), state 1 is the start;
``trans`` uint16 [S, 256], ``accept`` uint8 [S], S <= GUIDE_MAX_STATES.  States from which no
accepting state can be reached are folded into the dead state, so a live state always has a
continuation or is accepting.

Regular expressions are parsed by the standard library's parser.  Supported: literals, ``.``,
classes and negated classes, ``\\d \\s \\w`` (ASCII) and their negations, groups, alternation,
``? * +`` and ``{m,n}`` (greedy or lazy: the language is the same).  ``.`` and negated classes also
admit every well-formed multi-byte UTF-8 sequence.  The match is an implicit full match.  Refused with a
ValueError that names the construct: backreferences, lookaround, anchors, flags, possessive / atomic
groups.

JSON documents (``schema_regex``, ``json_object_regex``): at every structural gap (after ``{ [ , :``
and before ``} ]``) at most one space, no newlines; strings in JSON syntax.
"""

from __future__ import annotations

import hashlib
import json
import re
from dataclasses import dataclass

import numpy as np

try:  # Python >= 3.11
    import re._parser as _sre  # type: ignore
except ImportError:  # Python 3.10
    import sre_parse as _sre  # type: ignore

GUIDE_MAX_STATES = 4096
JSON_OBJECT_DEPTH = 4  # the values of a ``json_object`` answer nest at most this deep (containers inside the object)
CHOICE_MAX = 256
_NFA_MAX = 400_000  # NFA states: far above anything that still minimises under GUIDE_MAX_STATES
_DFA_MAX = 300_000  # DFA states before minimisation
_MAX_CP = 0x10FFFF


@dataclass(eq=False)
class Guide:
    """A compiled grammar: the DFA and the content hash the engine keeps it resident under."""

    trans: np.ndarray  # uint16 [S, 256]
    accept: np.ndarray  # uint8 [S]
    key: str

    @property
    def states(self) -> int:
        return int(self.trans.shape[0])

    def matches(self, data: bytes) -> bool:
        s = walk(self, 1, data)
        return bool(s) and bool(self.accept[s])


def walk(dfa: Guide, state: int, data: bytes) -> int:
    """The state after ``data`` from ``state`` (0: refused)."""
    t = dfa.trans
    for b in data:
        state = int(t[state, b])
        if state == 0:
            return 0
    return state


def advance(dfa: Guide, state: int, token_bytes: bytes) -> int:
    """Host-side stepping: the state after an emitted token's bytes (0: the token is not allowed)."""
    return walk(dfa, state, token_bytes)


# ------------------------------------------------------------------------------------------------
# code point sets -> UTF-8 byte sequences
# ------------------------------------------------------------------------------------------------
def _norm(ranges):
    """Sorted, merged code point ranges without the surrogates (not encodable in UTF-8)."""
    out = []
    for lo, hi in sorted(ranges):
        for a, b in ((lo, min(hi, 0xD7FF)), (max(lo, 0xE000), hi)):
            if a > b:
                continue
            if out and a <= out[-1][1] + 1:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
    return [(a, b) for a, b in out]


def _negate(ranges):
    out, nxt = [], 0
    for lo, hi in _norm(ranges):
        if lo > nxt:
            out.append((nxt, lo - 1))
        nxt = hi + 1
    if nxt <= _MAX_CP:
        out.append((nxt, _MAX_CP))
    return _norm(out)


def _utf8_seqs(lo: int, hi: int):
    """Sequences of byte ranges whose products are exactly the UTF-8 encodings of [lo, hi]."""
    for bound in (0x7F, 0x7FF, 0xFFFF):
        if lo <= bound < hi:
            yield from _utf8_seqs(lo, bound)
            yield from _utf8_seqs(bound + 1, hi)
            return
    if hi <= 0x7F:
        yield [(lo, hi)]
        return
    for i in (1, 2, 3):
        m = (1 << (6 * i)) - 1
        if lo & ~m != hi & ~m:
            if lo & m != 0:
                yield from _utf8_seqs(lo, lo | m)
                yield from _utf8_seqs((lo | m) + 1, hi)
                return
            if hi & m != m:
                yield from _utf8_seqs(lo, (hi & ~m) - 1)
                yield from _utf8_seqs(hi & ~m, hi)
                return
    a, b = chr(lo).encode("utf-8"), chr(hi).encode("utf-8")
    yield list(zip(a, b))


# ------------------------------------------------------------------------------------------------
# regex -> NFA
# ------------------------------------------------------------------------------------------------
_DIGIT = [(48, 57)]
_SPACE = [(9, 13), (32, 32)]
_WORD = [(48, 57), (65, 90), (95, 95), (97, 122)]


class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple]] = []  # per state: (lo byte, hi byte, target)

    def new(self) -> int:
        if len(self.eps) >= _NFA_MAX:
            raise ValueError(f"grammar too large: more than {_NFA_MAX} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def cpset(self, ranges, a: int, b: int):
        """Edges from a to b that spell one code point of ``ranges`` in UTF-8 (equal prefixes shared)."""
        heads: dict = {}
        for lo, hi in _norm(ranges):
            for seq in _utf8_seqs(lo, hi):
                cur = a
                for x, y in seq[:-1]:
                    nxt = heads.get((cur, x, y))
                    if nxt is None:
                        nxt = heads[cur, x, y] = self.new()
                        self.edges[cur].append((x, y, nxt))
                    cur = nxt
                self.edges[cur].append((*seq[-1], b))


def _category(cat):
    name = str(cat)
    table = {"CATEGORY_DIGIT": (_DIGIT, False), "CATEGORY_NOT_DIGIT": (_DIGIT, True),
             "CATEGORY_SPACE": (_SPACE, False), "CATEGORY_NOT_SPACE": (_SPACE, True),
             "CATEGORY_WORD": (_WORD, False), "CATEGORY_NOT_WORD": (_WORD, True)}
    if name not in table:
        raise ValueError(f"unsupported regex construct: {name.lower()}")
    r, neg = table[name]
    return _negate(r) if neg else r


def _build(nfa: _NFA, items, a: int, b: int):
    """Thompson construction of the parsed sequence ``items`` between states a and b."""
    cur = a
    items = list(items)
    for n, (op, av) in enumerate(items):
        nxt = b if n == len(items) - 1 else nfa.new()
        name = str(op)
        if name == "LITERAL":
            nfa.cpset([(av, av)], cur, nxt)
        elif name == "NOT_LITERAL":
            nfa.cpset(_negate([(av, av)]), cur, nxt)
        elif name == "ANY":
            nfa.cpset(_negate([(10, 10)]), cur, nxt)
        elif name == "IN":
            neg, ranges = False, []
            for o, v in av:
                o = str(o)
                if o == "NEGATE":
                    neg = True
                elif o == "LITERAL":
                    ranges.append((v, v))
                elif o == "RANGE":
                    ranges.append((v[0], v[1]))
                elif o == "CATEGORY":
                    ranges.extend(_category(v))
                else:
                    raise ValueError(f"unsupported regex construct in a class: {o.lower()}")
            nfa.cpset(_negate(ranges) if neg else ranges, cur, nxt)
        elif name == "SUBPATTERN":
            _, add_flags, del_flags, p = av
            if add_flags or del_flags:
                raise ValueError("unsupported regex construct: flags (inline flag group)")
            _build(nfa, p, cur, nxt)
        elif name == "BRANCH":
            for alt in av[1]:
                s, e = nfa.new(), nfa.new()
                nfa.eps[cur].append(s)
                nfa.eps[e].append(nxt)
                _build(nfa, alt, s, e)
        elif name in ("MAX_REPEAT", "MIN_REPEAT"):
            lo, hi, p = av
            unbounded = hi == _sre.MAXREPEAT
            at = cur
            for _ in range(lo):
                e = nfa.new()
                _build(nfa, p, at, e)
                at = e
            if unbounded:
                s, e = nfa.new(), nfa.new()
                nfa.eps[at].extend([s, nxt])
                _build(nfa, p, s, e)
                nfa.eps[e].extend([s, nxt])
            else:
                for _ in range(hi - lo):
                    e = nfa.new()
                    nfa.eps[at].append(nxt)
                    _build(nfa, p, at, e)
                    at = e
                nfa.eps[at].append(nxt)
        elif name == "AT":
            raise ValueError(f"unsupported regex construct: anchor ({str(av).lower()}); the match is always a full match")
        elif name in ("ASSERT", "ASSERT_NOT"):
            raise ValueError("unsupported regex construct: lookaround")
        elif name in ("GROUPREF", "GROUPREF_EXISTS"):
            raise ValueError("unsupported regex construct: backreference")
        elif name in ("POSSESSIVE_REPEAT", "ATOMIC_GROUP"):
            raise ValueError(f"unsupported regex construct: {name.lower()}")
        else:
            raise ValueError(f"unsupported regex construct: {name.lower()}")
        cur = nxt
    if not items:
        nfa.eps[a].append(b)


def _parse(pattern: str):
    if not isinstance(pattern, str):
        raise ValueError("a regex must be a string")
    try:
        p = _sre.parse(pattern, 0)
    except (re.error, RecursionError, OverflowError) as e:
        raise ValueError(f"invalid regex: {e}") from None
    flags = p.state.flags & ~re.UNICODE
    if flags:
        raise ValueError("unsupported regex construct: flags (global inline flags)")
    return p


# ------------------------------------------------------------------------------------------------
# NFA -> DFA -> minimised DFA
# ------------------------------------------------------------------------------------------------
def _closures(nfa: _NFA, final: int):
    """Per NFA state its epsilon closure, reduced to the states that matter to the subset
    construction: those with byte edges and the final state."""
    n = len(nfa.eps)
    clo: list = [None] * n
    for s in range(n):
        seen, stack = {s}, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        clo[s] = frozenset(t for t in seen if nfa.edges[t] or t == final)
    return clo


def _subset(nfa: _NFA, start: int, final: int):
    """(trans over byte intervals [S, C], accept [S], interval starts): DFA state 0 is dead, 1 the start."""
    clo = _closures(nfa, final)
    cuts = {0, 256}
    for es in nfa.edges:
        for lo, hi, _ in es:
            cuts.add(lo)
            cuts.add(hi + 1)
    cuts = sorted(cuts)
    first = {c: i for i, c in enumerate(cuts)}
    C = len(cuts) - 1
    # per NFA state: [(interval indices, closure of the target)]
    useful = [[(range(first[lo], first[hi + 1]), clo[t]) for lo, hi, t in es] for es in nfa.edges]
    s0 = clo[start]
    ids = {frozenset(): 0, s0: 1}
    order = [frozenset(), s0]
    rows = [[0] * C]
    i = 1
    while i < len(order):
        cur = order[i]
        i += 1
        tgt: dict = {}
        for s in cur:
            for idxs, dest in useful[s]:
                for k in idxs:
                    have = tgt.get(k)
                    tgt[k] = dest if have is None else (have if dest <= have else have | dest)
        row = [0] * C
        memo: dict = {}
        for k, dest in tgt.items():
            j = memo.get(id(dest))
            if j is None:
                j = ids.get(dest)
                if j is None:
                    if len(order) >= _DFA_MAX:
                        raise ValueError(f"grammar too large: more than {_DFA_MAX} states before minimisation")
                    j = ids[dest] = len(order)
                    order.append(dest)
                memo[id(dest)] = j
            row[k] = j
        rows.append(row)
    trans = np.asarray(rows, dtype=np.int32).reshape(len(order), C)
    accept = np.fromiter((final in s for s in order), dtype=bool, count=len(order))
    return trans, accept, cuts


def _prune(trans: np.ndarray, accept: np.ndarray):
    """Fold the states that cannot reach an accepting state into the dead state 0."""
    live = accept.copy()
    while True:
        new = live | live[trans].any(axis=1)
        if (new == live).all():
            break
        live = new
    live[0] = False
    keep = live.copy()
    keep[1] = True  # the start state stays state 1 even for the empty language
    remap = np.zeros(len(trans), dtype=np.int32)
    idx = np.flatnonzero(keep)
    idx = idx[idx != 0]
    remap[idx] = np.arange(1, len(idx) + 1, dtype=np.int32)
    t = np.zeros((len(idx) + 1, trans.shape[1]), dtype=np.int32)
    t[1:] = np.where(live[trans[idx]], remap[trans[idx]], 0)
    a = np.zeros(len(idx) + 1, dtype=bool)
    a[1:] = accept[idx]
    return t, a


def _minimise(trans: np.ndarray, accept: np.ndarray):
    """Moore partition refinement (exact: the signatures themselves are compared).  Keeps 0 dead, 1 start."""
    S = len(trans)
    # the dead state is its own block from the beginning: nothing else has all-dead rows and rejects
    label = accept.astype(np.int64) + 1
    label[0] = 0
    # dense labels 0 .. count - 1 (when every live state accepts, label 1 is unused): the pair key
    # below is injective only for labels below count
    _, label = np.unique(label, return_inverse=True)
    label = label.reshape(-1).astype(np.int64)
    count = int(label.max()) + 1
    cols = [np.ascontiguousarray(trans[:, c]) for c in range(trans.shape[1])]
    while True:
        # the signature (own block, block of every successor), folded in column by column: two states
        # share a block afterwards iff all of it agrees (exact: the pairs are renumbered, not hashed)
        new, n = label, count
        for col in cols:
            _, new = np.unique(new * count + label[col], return_inverse=True)
            new = new.reshape(-1)
            n = int(new.max()) + 1
        label = new
        if n == count:
            break
        count = n
    # renumber: block of state 0 -> 0, block of state 1 -> 1, the rest in order of first appearance
    new = np.full(count, -1, dtype=np.int64)
    new[label[0]] = 0
    if S > 1:
        new[label[1]] = 1 if label[1] != label[0] else 0
    nxt = 2
    rep = {int(label[0]): 0}
    if S > 1:
        rep.setdefault(int(label[1]), 1)
    for s in range(S):
        b = int(label[s])
        if new[b] < 0:
            new[b] = nxt
            nxt += 1
            rep[b] = s
    n_out = max(nxt, 2)
    t = np.zeros((n_out, trans.shape[1]), dtype=np.int32)
    a = np.zeros(n_out, dtype=bool)
    for b, s in rep.items():
        t[new[b]] = new[label[trans[s]]]
        a[new[b]] = accept[s]
    return t, a


def compile_regex(pattern: str, minimise: bool = True) -> Guide:
    """The DFA of ``pattern`` (full match over the UTF-8 bytes).  ValueError: an unsupported construct
    (named), an invalid pattern, or a grammar of more than GUIDE_MAX_STATES states."""
    parsed = _parse(pattern)
    nfa = _NFA()
    a, b = nfa.new(), nfa.new()
    try:
        _build(nfa, parsed, a, b)
    except RecursionError:
        raise ValueError("grammar too large: the regex nests too deeply") from None
    trans, accept, cuts = _subset(nfa, a, b)
    trans, accept = _prune(trans, accept)
    if minimise:
        trans, accept = _minimise(trans, accept)
    S = len(trans)
    if S > GUIDE_MAX_STATES:
        raise ValueError(f"grammar too large: {S} states (at most {GUIDE_MAX_STATES})")
    widths = np.diff(np.asarray(cuts))
    full = np.repeat(trans, widths, axis=1).astype(np.uint16)
    assert full.shape == (S, 256) and not full[0].any()
    acc = accept.astype(np.uint8)
    h = hashlib.sha256(full.tobytes() + b"\0" + acc.tobytes()).hexdigest()
    return Guide(np.ascontiguousarray(full), acc, h)


# ------------------------------------------------------------------------------------------------
# front ends: choice, JSON schema, json_object
# ------------------------------------------------------------------------------------------------
_WS = "[ ]?"
_CHAR = r'(?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})'
_STRING = f'"{_CHAR}*"'
_INTEGER = r"-?(?:0|[1-9][0-9]*)"
_NUMBER = _INTEGER + r"(?:\.[0-9]+)?(?:[eE][+-]?[0-9]+)?"
_SCALARS = f"{_STRING}|{_NUMBER}|true|false|null"


def choice_regex(choices) -> str:
    if (not isinstance(choices, (list, tuple)) or not 1 <= len(choices) <= CHOICE_MAX
            or not all(isinstance(c, str) and c for c in choices)):
        raise ValueError(f"guided_choice must be a list of 1 to {CHOICE_MAX} non-empty strings")
    return "|".join(re.escape(c) for c in choices)


def _array(item: str, lo: int = 0, hi: int | None = None) -> str:
    if hi is not None and hi < max(lo, 0):
        raise ValueError(f"minItems {lo} exceeds maxItems {hi}")
    if hi == 0:
        return rf"\[{_WS}\]"
    more = f"(?:,{_WS}{item}){{{max(lo - 1, 0)},{'' if hi is None else hi - 1}}}"
    body = f"{item}{more}{_WS}"
    return rf"\[{_WS}{body}\]" if lo > 0 else rf"\[{_WS}(?:{body})?\]"


def _value_regex(depth: int) -> str:
    """Any JSON value whose containers nest at most ``depth`` deep (0: scalars only)."""
    if depth <= 0:
        return f"(?:{_SCALARS})"
    return f"(?:{_SCALARS}|{_object_regex(depth)}|{_array(_value_regex(depth - 1))})"


def _object_regex(depth: int) -> str:
    member = f"{_STRING}:{_WS}{_value_regex(depth - 1)}"
    return rf"\{{{_WS}(?:{member}(?:,{_WS}{member})*{_WS})?\}}"


def json_object_regex(depth: int = JSON_OBJECT_DEPTH) -> str:
    """``response_format: {"type": "json_object"}``: any JSON object whose values nest at most ``depth``
    levels deep (a scalar: 0; ``{"a": {"b": [1]}}``: 2)."""
    return _object_regex(depth + 1)


_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "$defs", "definitions", "$comment"}
_TYPE_KEYS = {
    "object": {"properties", "required", "additionalProperties"},
    "array": {"items", "minItems", "maxItems"},
    "string": {"minLength", "maxLength", "pattern"},
    "integer": set(), "number": set(), "boolean": set(), "null": set(),
}
_GENERIC_DEPTH = 2  # nesting of a value the schema says nothing about (``{}``, an array without ``items``)


def _literal(v) -> str:
    if isinstance(v, (dict, list)):
        raise ValueError("enum / const: only JSON scalars are supported")
    forms = {json.dumps(v), json.dumps(v, ensure_ascii=False)}
    return "|".join(re.escape(f) for f in sorted(forms))


def _count(schema, key, default=None):
    v = schema.get(key, default)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"{key} must be a non-negative integer")
    return v


_RAW_STRING_BYTES = list(range(0x20)) + [0x22, 0x5C]  # control characters, the quote and the backslash


def _check_string_pattern(pat: str) -> None:
    """A string ``pattern`` is matched against the raw text between the quotes, so it must not be able
    to put a quote, a backslash or a control character there: the answer would no longer be JSON."""
    dfa = compile_regex(pat)  # (pruned: every state left is reachable and can still reach acceptance)
    hit = np.flatnonzero(dfa.trans[1:, _RAW_STRING_BYTES].any(axis=0))
    if len(hit):
        b = _RAW_STRING_BYTES[int(hit[0])]
        raise ValueError(f"unsupported schema keyword: pattern {pat!r} can match the byte 0x{b:02x} ({chr(b)!r}), "
                         "which a JSON string cannot hold unescaped; exclude quotes, backslashes and control "
                         "characters (e.g. [^\"\\\\\\x00-\\x1f] in place of .)")


def _schema_regex(schema, root, stack) -> str:
    if schema is True:
        return _value_regex(_GENERIC_DEPTH)
    if not isinstance(schema, dict):
        raise ValueError(f"a schema must be an object, got {type(schema).__name__}")
    if "$ref" in schema:
        ref = schema["$ref"]
        extra = set(schema) - _ANNOTATIONS - {"$ref"}
        if extra:
            raise ValueError(f"unsupported schema keyword next to $ref: {sorted(extra)[0]}")
        if not isinstance(ref, str) or not (ref.startswith("#/$defs/") or ref.startswith("#/definitions/")):
            raise ValueError(f"unsupported $ref {ref!r}: only #/$defs/NAME and #/definitions/NAME")
        if ref in stack:
            raise ValueError(f"unsupported schema: recursive $ref {ref!r}")
        _, table, name = ref.split("/", 2)
        target = (root.get(table) or {}).get(name) if isinstance(root, dict) else None
        if target is None:
            raise ValueError(f"$ref {ref!r} does not resolve")
        return _schema_regex(target, root, stack + (ref,))
    for comb in ("anyOf", "oneOf"):
        if comb in schema:
            extra = set(schema) - _ANNOTATIONS - {comb}
            if extra:
                raise ValueError(f"unsupported schema keyword next to {comb}: {sorted(extra)[0]}")
            alts = schema[comb]
            if not isinstance(alts, list) or not alts:
                raise ValueError(f"{comb} must be a non-empty list")
            return "(?:" + "|".join(_schema_regex(s, root, stack) for s in alts) + ")"
    if "enum" in schema or "const" in schema:
        extra = set(schema) - _ANNOTATIONS - {"enum", "const", "type"}
        if extra:
            raise ValueError(f"unsupported schema keyword next to enum / const: {sorted(extra)[0]}")
        vals = schema["enum"] if "enum" in schema else [schema["const"]]
        if not isinstance(vals, list) or not vals:
            raise ValueError("enum must be a non-empty list")
        return "(?:" + "|".join(_literal(v) for v in vals) + ")"
    types = schema.get("type")
    if types is None:
        extra = set(schema) - _ANNOTATIONS
        if extra:
            raise ValueError(f"unsupported schema keyword (without a type): {sorted(extra)[0]}")
        return _value_regex(_GENERIC_DEPTH)
    types = types if isinstance(types, list) else [types]
    allowed = set(_ANNOTATIONS) | {"type"}
    for t in types:
        if not isinstance(t, str) or t not in _TYPE_KEYS:
            raise ValueError(f"unsupported schema type: {t!r}")
        allowed |= _TYPE_KEYS[t]
    for k in schema:
        if k not in allowed:
            raise ValueError(f"unsupported schema keyword: {k}")
    out = []
    for t in types:
        if t == "string":
            lo, hi = _count(schema, "minLength", 0), _count(schema, "maxLength")
            if "pattern" in schema:
                if lo or hi is not None:
                    raise ValueError("unsupported schema keyword: pattern together with minLength / maxLength")
                pat = schema["pattern"]
                if not isinstance(pat, str):
                    raise ValueError("pattern must be a string")
                pat = pat[1:] if pat.startswith("^") else pat
                pat = pat[:-1] if pat.endswith("$") and not pat.endswith("\\$") else pat
                _check_string_pattern(pat)
                out.append(f'"(?:{pat})"')
            elif lo == 0 and hi is None:
                out.append(_STRING)
            else:
                if hi is not None and hi < lo:
                    raise ValueError(f"minLength {lo} exceeds maxLength {hi}")
                out.append(f'"{_CHAR}{{{lo},{"" if hi is None else hi}}}"')
        elif t == "integer":
            out.append(_INTEGER)
        elif t == "number":
            out.append(_NUMBER)
        elif t == "boolean":
            out.append("true|false")
        elif t == "null":
            out.append("null")
        elif t == "array":
            item = _schema_regex(schema["items"], root, stack) if "items" in schema else _value_regex(_GENERIC_DEPTH)
            out.append(_array(item, _count(schema, "minItems", 0), _count(schema, "maxItems")))
        elif t == "object":
            out.append(_object_schema_regex(schema, root, stack))
    return "(?:" + "|".join(out) + ")"


def _object_schema_regex(schema, root, stack) -> str:
    if schema.get("additionalProperties", False) is not False:
        raise ValueError("unsupported schema keyword: additionalProperties (only false: additional properties "
                         "are never emitted)")
    props = schema.get("properties", {})
    required = schema.get("required", [])
    if not isinstance(props, dict) or not isinstance(required, list):
        raise ValueError("properties must be an object and required a list")
    for r in required:
        if r not in props:
            raise ValueError(f"required names {r!r}, which is not in properties")
    members = [(f"{re.escape(json.dumps(k))}:{_WS}{_schema_regex(v, root, stack)}", k in required)
               for k, v in props.items()]
    n = len(members)
    # rest[i]: members i.. after something was emitted (each one brings its comma)
    rest = [""] * (n + 1)
    for i in range(n - 1, -1, -1):
        m, req = members[i]
        rest[i] = (f",{_WS}{m}" if req else f"(?:,{_WS}{m})?") + rest[i + 1]
    # first[i]: members i.. with nothing emitted yet; None: they may all be left out and this is "nothing"
    first = None
    for i in range(n - 1, -1, -1):
        m, req = members[i]
        here = m + rest[i + 1]
        if req:
            first = here
        else:
            first = here if first is None else f"(?:{here}|{first})"
    if first is None:
        return rf"\{{{_WS}\}}"
    if any(req for _, req in members):
        return rf"\{{{_WS}{first}{_WS}\}}"
    return rf"\{{{_WS}(?:{first}{_WS})?\}}"


def schema_regex(schema) -> str:
    """The regex of the documents that conform to ``schema`` (the supported JSON-Schema subset; a
    ValueError names any other constraining keyword)."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"the schema is not valid JSON: {e}") from None
    if not isinstance(schema, dict):
        raise ValueError("a schema must be an object")
    return _schema_regex(schema, schema, ())


def compile_choice(choices) -> Guide:
    return compile_regex(choice_regex(choices))


def compile_json_schema(schema) -> Guide:
    return compile_regex(schema_regex(schema))


def compile_json_object() -> Guide:
    return compile_regex(json_object_regex())


# ------------------------------------------------------------------------------------------------
# token byte tables
# ------------------------------------------------------------------------------------------------
def pack_token_bytes(table, vocab: int):
    """``(tok_off int32 [vocab + 1], tok_bytes uint8 [max(total, 1)])`` of a ``token_bytes()`` list;
    ids from ``len(table)`` up to the model's vocabulary size are empty."""
    table = list(table)[:vocab]
    lens = np.zeros(vocab, dtype=np.int64)
    lens[: len(table)] = [len(b) for b in table]
    off = np.zeros(vocab + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2**31:
        raise ValueError("token byte table too large")
    blob = np.frombuffer(b"".join(table) or b"\0", dtype=np.uint8).copy()
    return off.astype(np.int32), blob
