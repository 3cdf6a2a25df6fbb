"""Regular-expression constraints for generation, host side: a pattern becomes a deterministic automaton over BYTES (``ByteDFA``) and a
vocabulary becomes a table of every token's bytes (``TokenBytes``).  ``fused_ops.grammar_mask`` (csrc/grammar_mask.hip) walks both on the
device inside the decode step: a token is allowed when the automaton, from the row's current state, survives the token's bytes.

The guarantee is at the byte level: the concatenation of the generated ids' byte strings (end token excluded) is a viable prefix of the
pattern's language after every step - some continuation completes it - and a generation that ends on the end token is a full match.
An EMPTY token (control / unknown / unused pieces, the special tokens) is never allowed by a grammar.

Pattern syntax (full-match semantics; a leading ``^`` and a trailing ``$`` are accepted and ignored):
    literal characters (a non-ASCII literal is its UTF-8 bytes), escaped metacharacters, ``\\n \\t \\r \\f \\v \\0 \\xHH``
    ``\\d \\w \\s`` and ``\\D \\W \\S`` - the ASCII classes (Python's ``re.ASCII``)
    ``[...]`` classes with ASCII ranges, escapes and negation; ``.`` (anything but ``\\n``)
    ``( )``, ``(?: )`` (both only group), ``|``
    ``* + ? {m} {m,} {m,n} {,n}``
``.``, a negated class and ``\\D \\W \\S`` match every ASCII byte they do not exclude and every well-formed multi-byte UTF-8 sequence, so a
constrained output always decodes.  Everything else raises ``ValueError`` naming the construct: backreferences, lookaround, named groups,
flags, lazy and possessive quantifiers, anchors inside the pattern, ``\\b`` and its kin, non-ASCII characters in a range or a negated class.

Pipeline: parser (this module's own) -> Thompson NFA over bytes -> subset construction -> trimming (every kept state reaches an accepting
state: a live state can always finish) -> minimisation (Hopcroft) -> byte classes (bytes no state distinguishes share a column).

Limits, those of the kernel's LDS copy of the table: ``n_states * n_classes <= GRAMMAR_TABLE_MAX`` and ``n_states <= GRAMMAR_STATES_MAX``.

Past regular languages: ``BytePDA`` is a deterministic real-time pushdown automaton over bytes - one move per byte, no empty moves, one
bounded stack of at most three symbols - walked by ``fused_ops.pda_mask`` (csrc/pda_mask.hip); ``json_grammar`` builds the one for RFC
8259 JSON with arbitrary nesting (depth comes from the stack, not from the table), ``BytePDA.from_dfa`` lifts a ``ByteDFA`` (no stack
symbols, the same language), ``as_grammar`` takes a pattern string, a ``ByteDFA`` or a ``BytePDA``."""
from collections import deque

import numpy as np

GRAMMAR_TABLE_MAX = 16384     # entries of one row's transition table (uint16: 32 KB, LDS-resident under the default 64 KB limit)
GRAMMAR_STATES_MAX = 4095
DEAD = 0xFFFF                 # table entry: no transition
REPEAT_MAX = 4096             # the largest count in {m,n}: a bound is unrolled
PDA_DEPTH_MAX = 64            # symbols a row's stack holds (QL_PDA_DEPTH_MAX)
PDA_LOCAL_MAX = 32            # symbols ONE token's walk may hold above the lowest depth it reached (QL_PDA_LOCAL_MAX): the window rule
PDA_SYMS_MAX = 3              # stack symbols 1..n_syms (QL_PDA_SYMS_MAX); 0 = the empty stack read as top
PDA_DEAD = 0xFFFF             # BytePDA table entry: no move (next state 0xFFF, op 3)
PDA_NONE, PDA_POP, PDA_PUSH = 0, 1, 2

_ALL = (1 << 256) - 1
_ASCII = (1 << 128) - 1


def _mask(*items) -> int:
    """A byte set as a 256-bit integer: ints are bytes, (lo, hi) pairs inclusive ranges."""
    m = 0
    for it in items:
        if isinstance(it, tuple):
            m |= ((1 << (it[1] - it[0] + 1)) - 1) << it[0]
        else:
            m |= 1 << it
    return m


_DIGIT = _mask((0x30, 0x39))
_WORD = _DIGIT | _mask((0x41, 0x5A), (0x61, 0x7A), 0x5F)
_SPACE = _mask(0x20, (0x09, 0x0D))
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CHAR_ESC = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B, "0": 0x00}
NFA_STATES_MAX = 1 << 18      # nested bounded repeats multiply: past this the pattern is refused before it is determinised

# AST: ("set", mask) one byte of the set | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
_CONT = ("set", _mask((0x80, 0xBF)))
# every well-formed multi-byte UTF-8 sequence (Unicode table 3-7: no overlong forms, no surrogates, nothing past U+10FFFF)
_UTF8_MULTI = [
    ("cat", [("set", _mask((0xC2, 0xDF))), _CONT]),
    ("cat", [("set", _mask(0xE0)), ("set", _mask((0xA0, 0xBF))), _CONT]),
    ("cat", [("set", _mask((0xE1, 0xEC), 0xEE, 0xEF)), _CONT, _CONT]),
    ("cat", [("set", _mask(0xED)), ("set", _mask((0x80, 0x9F))), _CONT]),
    ("cat", [("set", _mask(0xF0)), ("set", _mask((0x90, 0xBF))), _CONT, _CONT]),
    ("cat", [("set", _mask((0xF1, 0xF3))), _CONT, _CONT, _CONT]),
    ("cat", [("set", _mask(0xF4)), ("set", _mask((0x80, 0x8F))), _CONT, _CONT]),
]


def _any_but(excluded_ascii: int):
    """One character outside an ASCII set: the other ASCII bytes, or any multi-byte sequence."""
    rest = _ASCII & ~excluded_ascii
    return ("alt", ([("set", rest)] if rest else []) + _UTF8_MULTI)


def _literal(ch: str):
    b = ch.encode("utf-8")
    if len(b) == 1:
        return ("set", 1 << b[0])
    return ("cat", [("set", 1 << v) for v in b])


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"compile_regex: the pattern must be a str (got {type(pattern).__name__})")
        self.full = pattern
        p = pattern
        if p.startswith("^"):
            p = p[1:]
        if p.endswith("$") and not self._escaped_end(p):
            p = p[:-1]
        self.p, self.i = p, 0

    @staticmethod
    def _escaped_end(p: str) -> bool:
        n = 0
        while n + 1 < len(p) and p[len(p) - 2 - n] == "\\":
            n += 1
        return n % 2 == 1

    def fail(self, what: str):
        raise ValueError(f"compile_regex: {what} is not supported (pattern {self.full!r})")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alternation()
        if self.i < len(self.p):
            raise ValueError(f"compile_regex: unbalanced ')' at {self.i} in {self.full!r}")
        return node

    def alternation(self):
        branches = [self.sequence()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.sequence())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def sequence(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        atom = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                lo, hi = self.braces()
                self.i -= 1                                     # (braces() stands behind the '}' already)
            else:
                return atom
            self.i += 1
            if self.peek() == "?":
                self.fail("a lazy quantifier")
            if self.peek() == "+":
                self.fail("a possessive quantifier")
            atom = ("rep", atom, lo, hi)

    def braces(self):
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else None
        parts = body.split(",") if body is not None else []
        if body is None or len(parts) > 2 or any(s and not s.isdigit() for s in parts) or (len(parts) == 1 and not parts[0]) or body == ",":
            raise ValueError(f"compile_regex: a malformed {{m,n}} quantifier at {self.i} in {self.full!r} (escape a literal brace)")
        lo = int(parts[0]) if parts[0] else 0
        hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if hi is not None and hi < lo:
            raise ValueError(f"compile_regex: {{{body}}}: the maximum is below the minimum in {self.full!r}")
        if max(lo, hi or 0) > REPEAT_MAX:
            raise ValueError(f"compile_regex: {{{body}}}: a repeat count above {REPEAT_MAX} in {self.full!r}")
        self.i = j + 1
        return lo, hi

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt.startswith(":"):
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("lookaround")
                elif nxt.startswith("P") or nxt.startswith("<"):
                    self.fail("a named group or a named backreference")
                elif nxt.startswith("#"):
                    self.fail("a comment group")
                elif nxt.startswith("("):
                    self.fail("a conditional group")
                else:
                    self.fail("an inline flag")
            node = self.alternation()
            if self.peek() != ")":
                raise ValueError(f"compile_regex: a missing ')' in {self.full!r}")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            return _any_but(1 << 0x0A)
        if c == "\\":
            kind, v = self.escape(in_class=False)
            return ("set", v) if kind == "set" else (_any_but(v) if kind == "neg" else _literal(v))
        if c in "*+?":
            raise ValueError(f"compile_regex: nothing to repeat at {self.i - 1} in {self.full!r}")
        if c == "{":
            raise ValueError(f"compile_regex: nothing to repeat at {self.i - 1} in {self.full!r} (escape a literal brace)")
        if c in "^$":
            self.fail("an anchor inside the pattern")
        return _literal(c)

    def escape(self, in_class: bool):
        """Behind a backslash: ("set", mask) / ("neg", excluded ASCII mask) / ("chr", character)."""
        c = self.peek()
        if c is None:
            raise ValueError(f"compile_regex: a trailing backslash in {self.full!r}")
        self.i += 1
        if c in _CLASS_ESC:
            return "set", _CLASS_ESC[c]
        if c.lower() in _CLASS_ESC and c.isupper():
            return "neg", _CLASS_ESC[c.lower()]
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(d not in "0123456789abcdefABCDEF" for d in h) or int(h, 16) > 0x7F:
                raise ValueError(f"compile_regex: \\x takes two hex digits of an ASCII byte in {self.full!r}")
            self.i += 2
            return "chr", chr(int(h, 16))
        if c in _CHAR_ESC:
            return "chr", chr(_CHAR_ESC[c])
        if c.isdigit():
            self.fail("a backreference")
        if c in "bBAZzG":
            self.fail(f"the assertion \\{c}")
        if c in "uUNpPkK":
            self.fail(f"the escape \\{c}")
        if c.isalnum():
            self.fail(f"the escape \\{c}")
        return "chr", c

    def char_class(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        mask, multi, first = 0, [], True
        while True:
            c = self.peek()
            if c is None:
                raise ValueError(f"compile_regex: a missing ']' in {self.full!r}")
            self.i += 1
            if c == "]" and not first:
                break
            first = False
            if c == "[" and self.peek() == ":":
                self.fail("a POSIX class")
            if c == "\\":
                kind, v = self.escape(in_class=True)
                if kind == "set":
                    mask |= v
                    continue
                if kind == "neg":
                    self.fail("a negated escape inside a class")
                c = v
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                self.i += 1
                hi = self.peek()
                self.i += 1
                if hi == "\\":
                    kind, hi = self.escape(in_class=True)
                    if kind != "chr":
                        raise ValueError(f"compile_regex: a class escape as the end of a range in {self.full!r}")
                if ord(c) > 0x7F or ord(hi) > 0x7F:
                    self.fail("a non-ASCII range inside a class")
                if ord(hi) < ord(c):
                    raise ValueError(f"compile_regex: the range {c}-{hi} is reversed in {self.full!r}")
                mask |= _mask((ord(c), ord(hi)))
            elif ord(c) > 0x7F:
                if negate:
                    self.fail("a non-ASCII character inside a negated class")
                multi.append(_literal(c))
            else:
                mask |= 1 << ord(c)
        if negate:
            return _any_but(mask)
        alts = ([("set", mask)] if mask else []) + multi
        return alts[0] if len(alts) == 1 else ("alt", alts)


class _NFA:
    def __init__(self):
        self.eps, self.trans = [], []            # per state: epsilon targets; (mask, target) pairs

    def state(self) -> int:
        if len(self.eps) >= NFA_STATES_MAX:
            raise ValueError(f"compile_regex: the pattern unrolls to more than {NFA_STATES_MAX} NFA states (nested bounded repeats)")
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node):
        """Thompson fragment of ``node``: (start, end), ``end`` without outgoing edges."""
        kind = node[0]
        if kind == "set":
            s, e = self.state(), self.state()
            if node[1]:
                self.trans[s].append((node[1], e))
            return s, e
        if kind == "cat":
            s = e = self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.state(), self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, item, lo, hi = node
        s = e = self.state()
        for _ in range(lo):
            a, b = self.build(item)
            self.eps[e].append(a)
            e = b
        if hi is None:                                          # a loop: e -> item -> back to e, or on
            a, b = self.build(item)
            out = self.state()
            self.eps[e] += [a, out]
            self.eps[b] += [a, out]
            return s, out
        out = self.state()
        for _ in range(hi - lo):                                # optional copies, each may leave
            a, b = self.build(item)
            self.eps[e] += [a, out]
            e = b
        self.eps[e].append(out)
        return s, out


def _byte_classes(masks):
    """Partition of the 256 bytes by which of ``masks`` hold them: (class_of list, one representative byte per class)."""
    masks = sorted(set(masks))
    sig_of, class_of, reps = {}, [0] * 256, []
    for b in range(256):
        sig = tuple((m >> b) & 1 for m in masks)
        c = sig_of.get(sig)
        if c is None:
            c = sig_of[sig] = len(reps)
            reps.append(b)
        class_of[b] = c
    return class_of, reps


def _determinize(nfa: _NFA, start: int, end: int, limit: int):
    """Subset construction over the NFA's byte classes.  Returns (rows, accept, class_of): rows[s][c] = next state or -1."""
    class_of, reps = _byte_classes([m for t in nfa.trans for m, _ in t])

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    first = closure([start])
    index, order, rows = {first: 0}, [first], []
    k = 0
    while k < len(order):
        cur, row = order[k], []
        k += 1
        for r in reps:
            bit = 1 << r
            nxt = {t for s in cur for m, t in nfa.trans[s] if m & bit}
            if not nxt:
                row.append(-1)
                continue
            nxt = closure(nxt)
            j = index.get(nxt)
            if j is None:
                j = index[nxt] = len(order)
                order.append(nxt)
                if len(order) > limit:
                    raise ValueError(f"compile_regex: the automaton has more than {limit} states before minimisation "
                                     f"(at most {GRAMMAR_STATES_MAX} states, GRAMMAR_STATES_MAX, after it)")
            row.append(j)
        rows.append(row)
    return rows, [end in s for s in order], class_of


def _trim(rows, accept):
    """Drop every state that reaches no accepting state (edges into one become -1) and every state the start does not reach; the
    start stays state 0.  Returns (rows, accept), or ([], []) when the start itself is dropped."""
    n = len(rows)
    back = [[] for _ in range(n)]
    for s, row in enumerate(rows):
        for t in row:
            if t >= 0:
                back[t].append(s)
    alive = [bool(a) for a in accept]
    stack = [s for s in range(n) if alive[s]]
    while stack:
        for p in back[stack.pop()]:
            if not alive[p]:
                alive[p] = True
                stack.append(p)
    if not n or not alive[0]:
        return [], []
    new, order, queue = {0: 0}, [0], deque([0])
    while queue:                                                # breadth first from the start: a canonical numbering
        for t in rows[queue.popleft()]:
            if t >= 0 and alive[t] and t not in new:
                new[t] = len(order)
                order.append(t)
                queue.append(t)
    out = [[new[t] if t >= 0 and alive[t] else -1 for t in rows[s]] for s in order]
    return out, [accept[s] for s in order]


def _minimize_rows(rows, accept):
    """Hopcroft's partition refinement on a trimmed automaton (a missing edge goes to an implicit sink); (rows, accept), start 0."""
    n = len(rows)
    if n == 0:
        return rows, accept
    C = len(rows[0])
    sink = n
    inv = [[[] for _ in range(n + 1)] for _ in range(C)]        # inv[c][t] = the states that go to t on c
    for s, row in enumerate(rows):
        for c, t in enumerate(row):
            inv[c][sink if t < 0 else t].append(s)
    for c in range(C):
        inv[c][sink].append(sink)
    acc = {s for s in range(n) if accept[s]}
    blocks = [b for b in (acc, set(range(n + 1)) - acc) if b]
    block_of = [0] * (n + 1)
    for i, b in enumerate(blocks):
        for s in b:
            block_of[s] = i
    work = deque((i, c) for i in range(len(blocks)) for c in range(C))
    queued = set(work)
    while work:
        i, c = work.popleft()
        queued.discard((i, c))
        pre = {}
        for t in blocks[i]:
            for s in inv[c][t]:
                pre.setdefault(block_of[s], set()).add(s)
        for j, part in pre.items():
            if len(part) == len(blocks[j]):
                continue
            rest = blocks[j] - part
            small, large = (part, rest) if len(part) <= len(rest) else (rest, part)
            blocks[j] = large
            k = len(blocks)
            blocks.append(small)
            for s in small:
                block_of[s] = k
            for cc in range(C):                                 # (j, cc) queued: both halves must be; otherwise the smaller half is
                work.append((k, cc))                            # enough (Hopcroft) - either way the new, smaller block goes in
                queued.add((k, cc))
    dead = block_of[sink]
    merged = [[-1 if t < 0 or block_of[t] == dead else block_of[t] for t in rows[next(iter(b - {sink}))]] if i != dead else None
              for i, b in enumerate(blocks)]
    # renumber breadth first from the start's block
    new, order, queue = {block_of[0]: 0}, [block_of[0]], deque([block_of[0]])
    while queue:
        for t in merged[queue.popleft()]:
            if t >= 0 and t not in new:
                new[t] = len(order)
                order.append(t)
                queue.append(t)
    out = [[new[t] if t >= 0 else -1 for t in merged[i]] for i in order]
    return out, [next(iter(blocks[i] - {sink})) in acc for i in order]


class ByteDFA:
    """A trimmed, minimal deterministic automaton over bytes.  ``n_states``, ``n_classes``; ``class_of`` (256,) uint8: a byte's column;
    ``table`` (n_states, n_classes) uint16: the next state or ``DEAD``; ``accept`` (n_states,) uint8 flags.  The start state is 0; every
    state reaches an accepting one.  ``pattern``: what it was compiled from, when known."""

    def __init__(self, class_of, table, accept, pattern=None):
        self.class_of = np.ascontiguousarray(class_of, dtype=np.uint8)
        self.table = np.ascontiguousarray(table, dtype=np.uint16)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        self.n_states, self.n_classes = self.table.shape
        self.pattern = pattern
        if self.class_of.shape != (256,) or self.accept.shape != (self.n_states,) or self.n_states < 1 or self.n_classes < 1:
            raise ValueError("ByteDFA: class_of (256,), table (n_states, n_classes), accept (n_states,)")
        if int(self.class_of.max()) >= self.n_classes:
            raise ValueError("ByteDFA: class_of names a column the table does not have")
        if self.n_states > GRAMMAR_STATES_MAX or self.n_states * self.n_classes > GRAMMAR_TABLE_MAX:
            raise ValueError(f"grammar too large: {self.n_states} states x {self.n_classes} byte classes = {self.n_states * self.n_classes} "
                             f"table entries (at most {GRAMMAR_TABLE_MAX} entries, GRAMMAR_TABLE_MAX, and {GRAMMAR_STATES_MAX} states, "
                             f"GRAMMAR_STATES_MAX)" + (f": pattern {pattern!r}" if pattern is not None else ""))
        self._rows = self.table.tolist()
        self._cls = self.class_of.tolist()

    start = 0

    def step(self, state: int, b: bytes) -> int:
        """The state after ``b`` from ``state``; -1 = dead (and a dead state stays dead)."""
        s = int(state)
        if not 0 <= s < self.n_states:
            return -1
        for v in bytes(b):
            s = self._rows[s][self._cls[v]]
            if s == DEAD:
                return -1
        return s

    def matches(self, b: bytes) -> bool:
        s = self.step(0, b)
        return s >= 0 and bool(self.accept[s])

    def accepting(self, state: int) -> bool:
        return 0 <= int(state) < self.n_states and bool(self.accept[int(state)])

    @staticmethod
    def from_choices(choices) -> "ByteDFA":
        """The language of exactly the given strings: an alternation of escaped literals."""
        choices = list(choices)
        if not choices or any(not isinstance(c, str) or not c for c in choices):
            raise ValueError("ByteDFA.from_choices: a non-empty list of non-empty strings")
        return compile_regex("|".join(escape(c) for c in choices))

    def __repr__(self):
        return f"ByteDFA({self.n_states} states x {self.n_classes} byte classes" + (f", {self.pattern!r})" if self.pattern is not None else ")")


def escape(text: str) -> str:
    """``text`` as a pattern that matches exactly it."""
    return "".join("\\" + c if c in "\\.[](){}|*+?^$" else ("\\n" if c == "\n" else c) for c in text)


def _finish(rows, accept, class_of, pattern) -> ByteDFA:
    """Trimmed minimal rows over some byte classes -> the ByteDFA: columns no state distinguishes are merged."""
    cols, col_of, keep = {}, [], []
    for c in range(len(rows[0])):
        key = tuple(row[c] for row in rows)
        if key not in cols:
            cols[key] = len(keep)
            keep.append(c)
        col_of.append(cols[key])
    # a byte class no byte belongs to any more cannot exist here (every class has a representative), but columns may repeat
    used = sorted({col_of[c] for c in class_of})
    renum = {c: i for i, c in enumerate(used)}
    table = [[DEAD if row[keep[c]] < 0 else row[keep[c]] for c in used] for row in rows]
    return ByteDFA([renum[col_of[c]] for c in class_of], np.array(table, dtype=np.uint16).reshape(len(rows), len(used)),
                   [1 if a else 0 for a in accept], pattern)


def compile_regex(pattern: str) -> ByteDFA:
    """Compile ``pattern`` (the module's comment lists the syntax) under full-match semantics.  ``ValueError`` for an unsupported
    construct (named), a malformed pattern, a pattern that matches nothing and a pattern whose automaton does not fit the limits (both
    numbers named)."""
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, end = nfa.build(ast)
    rows, accept, class_of = _determinize(nfa, start, end, limit=8 * GRAMMAR_TABLE_MAX)
    rows, accept = _trim(rows, accept)
    if not rows:
        raise ValueError(f"compile_regex: {pattern!r} matches nothing")
    rows, accept = _minimize_rows(rows, accept)
    return _finish(rows, accept, class_of, pattern)


def minimize(dfa: ByteDFA) -> ByteDFA:
    """Trim and minimise again (a compiled ByteDFA comes back equal: the construction is idempotent)."""
    rows = [[-1 if t == DEAD else t for t in row] for row in dfa.table.tolist()]
    rows, accept = _trim(rows, [bool(a) for a in dfa.accept.tolist()])
    if not rows:
        raise ValueError("minimize: the automaton accepts nothing")
    rows, accept = _minimize_rows(rows, accept)
    return _finish(rows, accept, dfa.class_of.tolist(), dfa.pattern)


def as_dfa(grammar) -> ByteDFA:
    """A ``ByteDFA`` as it is, a pattern string compiled."""
    if isinstance(grammar, ByteDFA):
        return grammar
    if isinstance(grammar, str):
        return compile_regex(grammar)
    raise ValueError(f"grammar: a ByteDFA or a pattern string (got {type(grammar).__name__})")


def pda_entry(nxt: int, op: int = PDA_NONE, sym: int = 0) -> int:
    """One ``BytePDA`` table entry: bits 0 - 11 the next state, bits 12 - 13 the op (0 none, 1 pop, 2 push, 3 dead), bits 14 - 15 the
    pushed symbol."""
    return (nxt & 0xFFF) | (op & 3) << 12 | (sym & 3) << 14


class BytePDA:
    """A deterministic real-time pushdown automaton over bytes: one move per byte, no empty moves, one stack of symbols 1..``n_syms``
    (``n_syms`` in 0..PDA_SYMS_MAX) that holds at most ``max_depth`` (<= PDA_DEPTH_MAX) of them.  ``class_of`` (256,) uint8: a byte's
    column; ``table`` (n_states, n_syms + 1, n_classes) uint16, flat index ``((state * (n_syms + 1) + top) * n_classes + class)`` where
    ``top`` is 0 for an empty stack and otherwise the symbol on top; ``accept`` (n_states,) uint8 flags.  An entry (``pda_entry``): bits
    0 - 11 the next state (0xFFF and anything >= n_states: dead), bits 12 - 13 the op (0 none, 1 pop, 2 push, 3 dead), bits 14 - 15 the
    pushed symbol.  A pop of an empty stack is dead, a push of symbol 0 or of one above ``n_syms`` is dead, a push onto a stack of
    ``max_depth`` symbols is dead.  The start configuration is state 0 with an empty stack; a configuration accepts when its state is
    accepting AND its stack is empty.  A configuration is ``(state, tuple of symbols, bottom first)``, or None = dead."""

    start = (0, ())

    def __init__(self, class_of, table, accept, n_syms: int, max_depth: int, name=None):
        self.n_syms, self.max_depth, self.name = int(n_syms), int(max_depth), name
        if not 0 <= self.n_syms <= PDA_SYMS_MAX:
            raise ValueError(f"BytePDA: n_syms {n_syms} outside 0..{PDA_SYMS_MAX} (PDA_SYMS_MAX)")
        if not 0 <= self.max_depth <= PDA_DEPTH_MAX:
            raise ValueError(f"BytePDA: max_depth {max_depth} outside 0..{PDA_DEPTH_MAX} (PDA_DEPTH_MAX)")
        self.class_of = np.ascontiguousarray(class_of, dtype=np.uint8)
        self.table = np.ascontiguousarray(table, dtype=np.uint16)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        if self.table.ndim != 3 or self.table.shape[1] != self.n_syms + 1 or self.table.shape[0] < 1 or self.table.shape[2] < 1:
            raise ValueError("BytePDA: table (n_states, n_syms + 1, n_classes)")
        self.n_states, _, self.n_classes = self.table.shape
        if self.class_of.shape != (256,) or self.accept.shape != (self.n_states,):
            raise ValueError("BytePDA: class_of (256,), accept (n_states,)")
        if int(self.class_of.max()) >= self.n_classes:
            raise ValueError("BytePDA: class_of names a column the table does not have")
        entries = self.n_states * (self.n_syms + 1) * self.n_classes
        if self.n_states > GRAMMAR_STATES_MAX or entries > GRAMMAR_TABLE_MAX:
            raise ValueError(f"grammar too large: {self.n_states} states x {self.n_syms + 1} stack tops x {self.n_classes} byte classes = "
                             f"{entries} table entries (at most {GRAMMAR_TABLE_MAX} entries, GRAMMAR_TABLE_MAX, and {GRAMMAR_STATES_MAX} "
                             f"states, GRAMMAR_STATES_MAX)")
        self._flat = self.table.reshape(-1).tolist()
        self._cls = self.class_of.tolist()

    def step(self, config, b: bytes, window=None):
        """The configuration after ``b`` from ``config``; None = dead (and dead stays dead).  ``window`` (the kernel walks one token with
        PDA_LOCAL_MAX): dead as soon as the walk holds more than that many symbols above the lowest depth it has reached."""
        if config is None:
            return None
        s, stack = int(config[0]), list(config[1])
        if not 0 <= s < self.n_states or len(stack) > self.max_depth or any(not 1 <= y <= self.n_syms for y in stack):
            return None
        low = len(stack)
        for v in bytes(b):
            top = stack[-1] if stack else 0
            e = self._flat[(s * (self.n_syms + 1) + top) * self.n_classes + self._cls[v]]
            nxt, op, sym = e & 0xFFF, (e >> 12) & 3, e >> 14
            if nxt >= self.n_states or op == 3:
                return None
            if op == PDA_POP:
                if not stack:
                    return None
                stack.pop()
                low = min(low, len(stack))
            elif op == PDA_PUSH:
                if sym == 0 or sym > self.n_syms or len(stack) == self.max_depth:
                    return None
                stack.append(sym)
                if window is not None and len(stack) - low > window:
                    return None
            s = nxt
        return s, tuple(stack)

    def matches(self, b: bytes) -> bool:
        return self.accepting(self.step(self.start, b))

    def accepting(self, config) -> bool:
        return config is not None and 0 <= int(config[0]) < self.n_states and bool(self.accept[int(config[0])]) and len(config[1]) == 0

    @staticmethod
    def from_dfa(dfa: "ByteDFA") -> "BytePDA":
        """``dfa`` as a pushdown automaton without stack symbols: the same states, the same language."""
        if not isinstance(dfa, ByteDFA):
            raise ValueError(f"BytePDA.from_dfa: a ByteDFA (got {type(dfa).__name__})")
        t = dfa.table.astype(np.uint16)                          # (a state is at most 4 094: bits 12 - 15 are 0 = no op)
        t = np.where(t == DEAD, np.uint16(PDA_DEAD), t).reshape(dfa.n_states, 1, dfa.n_classes)
        return BytePDA(dfa.class_of, t, dfa.accept, 0, 0, name=dfa.pattern)

    def __repr__(self):
        return (f"BytePDA({self.n_states} states x {self.n_syms + 1} stack tops x {self.n_classes} byte classes, depth <= {self.max_depth}"
                + (f", {self.name!r})" if self.name is not None else ")"))


_HEX = _mask((0x30, 0x39), (0x41, 0x46), (0x61, 0x66))
_WS = _mask(0x20, 0x09, 0x0A, 0x0D)
_SYM_ARRAY, _SYM_OBJECT = 1, 2


def json_grammar(root: str = "value", whitespace: bool = False, max_depth: int = 16) -> BytePDA:
    """The ``BytePDA`` of RFC 8259 JSON, built by hand.  ``root``: "value" (any JSON text), "object" or "array" (the text must be
    one).  Objects and arrays nest up to ``max_depth`` (<= PDA_DEPTH_MAX) levels; strings are well-formed UTF-8 without raw bytes below
    0x20, the escapes are ``\\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX``; numbers are ``-?(0|[1-9][0-9]*)(\\.[0-9]+)?([eE][+-]?[0-9]+)?``; the
    literals ``true false null``.  ``whitespace`` False: no whitespace outside strings (``json.dumps(..., separators=(",", ":"))``); True:
    ``[ \\t\\n\\r]*`` wherever JSON allows it.

    Two stack symbols, one per open container: array and object.  Every move is a single one: "[" and "{" push, "]" and "}" pop, a ","
    is dispatched on the top symbol (array: a value follows, object: a key), and a number - the one value without a closing byte of
    its own - is ended by the "," / "]" / "}" (or whitespace) behind it, which makes in the number's states the move it makes behind
    any other value."""
    if root not in ("value", "object", "array"):
        raise ValueError(f"json_grammar: root 'value', 'object' or 'array' (got {root!r})")
    if not isinstance(max_depth, int) or not 0 <= max_depth <= PDA_DEPTH_MAX:
        raise ValueError(f"json_grammar: max_depth {max_depth!r} outside 0..{PDA_DEPTH_MAX} (PDA_DEPTH_MAX)")
    names, moves = [], {}                                       # moves[(state, top, byte)] = (next state, op, symbol)
    tops = (0, _SYM_ARRAY, _SYM_OBJECT)

    def state(name):
        names.append(name)
        return name

    def on(src, byte_mask, dst, op=PDA_NONE, sym=0, top=tops):
        for t in top:
            for v in range(256):
                if (byte_mask >> v) & 1:
                    assert (src, t, v) not in moves, (src, t, v)
                    moves[(src, t, v)] = (dst, op, sym)

    def ch(text):
        return _mask(*text.encode())

    ws = _WS if whitespace else 0
    first = state("root") if root != "value" else None
    VAL, ARR0, OBJ0, KEY, COLON, AFTER = (state(n) for n in ("value", "array-open", "object-open", "key", "colon", "after"))

    def string(prefix, done):
        """The states of one string behind its opening quote; the closing quote goes to ``done``."""
        S, E, U1, U2, U3, U4, C1, C2, C3, E0, ED, F0, F4 = (state(prefix + n) for n in
                                                             ("str", "esc", "u1", "u2", "u3", "u4", "c1", "c2", "c3", "e0", "ed", "f0", "f4"))
        on(S, _mask((0x20, 0x7F)) & ~ch('"\\'), S)
        on(S, ch('"'), done)
        on(S, ch("\\"), E)
        on(E, ch('"\\/bfnrt'), S)
        on(E, ch("u"), U1)
        for a, b in ((U1, U2), (U2, U3), (U3, U4), (U4, S)):
            on(a, _HEX, b)
        # well-formed UTF-8 (Unicode table 3-7), as _UTF8_MULTI has it
        cont = _mask((0x80, 0xBF))
        on(S, _mask((0xC2, 0xDF)), C1)
        on(S, _mask(0xE0), E0)
        on(S, _mask((0xE1, 0xEC), 0xEE, 0xEF), C2)
        on(S, _mask(0xED), ED)
        on(S, _mask(0xF0), F0)
        on(S, _mask((0xF1, 0xF3)), C3)
        on(S, _mask(0xF4), F4)
        on(C1, cont, S)
        on(C2, cont, C1)
        on(C3, cont, C2)
        on(E0, _mask((0xA0, 0xBF)), C1)
        on(ED, _mask((0x80, 0x9F)), C1)
        on(F0, _mask((0x90, 0xBF)), C2)
        on(F4, _mask((0x80, 0x8F)), C2)
        return S

    KSTR, VSTR = string("key-", COLON), string("", AFTER)
    NEG, ZERO, INT, FRAC0, FRAC, EXP0, EXPS, EXP = (state(n) for n in ("minus", "zero", "int", "point", "frac", "e", "e-sign", "exp"))
    digit = _mask((0x30, 0x39))

    def value_start(src):
        on(src, ch('"'), VSTR)
        on(src, ch("-"), NEG)
        on(src, ch("0"), ZERO)
        on(src, _mask((0x31, 0x39)), INT)
        on(src, ch("["), ARR0, PDA_PUSH, _SYM_ARRAY)
        on(src, ch("{"), OBJ0, PDA_PUSH, _SYM_OBJECT)
        for word in ("true", "false", "null"):
            on(src, ch(word[0]), word + "1")

    def value_end(src):
        """Behind a complete value: "," and the closer of the container on top; with an empty stack nothing but whitespace."""
        on(src, ch(","), VAL, top=(_SYM_ARRAY,))
        on(src, ch("]"), AFTER, PDA_POP, top=(_SYM_ARRAY,))
        on(src, ch(","), KEY, top=(_SYM_OBJECT,))
        on(src, ch("}"), AFTER, PDA_POP, top=(_SYM_OBJECT,))
        on(src, ws, AFTER)

    for word in ("true", "false", "null"):
        for i in range(1, len(word)):
            state(word + str(i))
        for i in range(1, len(word)):
            on(word + str(i), ch(word[i]), word + str(i + 1) if i + 1 < len(word) else AFTER)
    if first is not None:
        on(first, ws, first)
        if root == "object":
            on(first, ch("{"), OBJ0, PDA_PUSH, _SYM_OBJECT)
        else:
            on(first, ch("["), ARR0, PDA_PUSH, _SYM_ARRAY)
    value_start(VAL)
    on(VAL, ws, VAL)
    value_start(ARR0)
    on(ARR0, ws, ARR0)
    on(ARR0, ch("]"), AFTER, PDA_POP, top=(_SYM_ARRAY,))
    on(OBJ0, ws, OBJ0)
    on(OBJ0, ch('"'), KSTR)
    on(OBJ0, ch("}"), AFTER, PDA_POP, top=(_SYM_OBJECT,))
    on(KEY, ws, KEY)
    on(KEY, ch('"'), KSTR)
    on(COLON, ws, COLON)
    on(COLON, ch(":"), VAL)
    value_end(AFTER)
    on(NEG, ch("0"), ZERO)
    on(NEG, _mask((0x31, 0x39)), INT)
    on(INT, digit, INT)
    for src in (ZERO, INT):
        on(src, ch("."), FRAC0)
    on(FRAC0, digit, FRAC)
    on(FRAC, digit, FRAC)
    for src in (ZERO, INT, FRAC):
        on(src, ch("eE"), EXP0)
    on(EXP0, ch("+-"), EXPS)
    for src in (EXP0, EXPS, EXP):
        on(src, digit, EXP)
    for src in (ZERO, INT, FRAC, EXP):
        value_end(src)
    # Every reachable configuration at a depth <= max_depth can finish, without a push: inside a string, a number, a literal or an
    # escape some byte completes the token (the closing quote, a digit, the literal's next letter, a hex digit, a continuation byte);
    # where a value is expected "0" is one; where a key is expected '"":0' is a member; behind a value the closer of the container on
    # top is a move (the top symbol always names the container the state is in, so the closer that pops it is the one defined) and
    # leaves a complete value one level down; with an empty stack "after" and the complete-number states accept.  max_depth only
    # refuses pushes, and no state needs one.  (With root "object" / "array" and max_depth 0 the root state cannot push: the language
    # is empty, as asked for.)
    index = {n: i for i, n in enumerate(names)}
    assert len(index) == len(names) and all(dst in index for dst, _, _ in moves.values())
    n = len(names)
    full = np.full((n, 3, 256), PDA_DEAD, dtype=np.uint16)
    for (src, t, v), (dst, op, sym) in moves.items():
        full[index[src], t, v] = pda_entry(index[dst], op, sym)
    cols, class_of, keep = {}, [], []
    for v in range(256):                                        # byte classes: bytes no (state, top) distinguishes share a column
        key = full[:, :, v].tobytes()
        if key not in cols:
            cols[key] = len(keep)
            keep.append(v)
        class_of.append(cols[key])
    accept = [1 if s in (AFTER, ZERO, INT, FRAC, EXP) else 0 for s in names]
    return BytePDA(class_of, full[:, :, keep], accept, 2, max_depth, name=f"json({root}{', whitespace' if whitespace else ''})")


def as_grammar(grammar):
    """A ``ByteDFA`` or a ``BytePDA`` as it is, a pattern string compiled (to a ``ByteDFA``)."""
    if isinstance(grammar, (ByteDFA, BytePDA)):
        return grammar
    if isinstance(grammar, str):
        return compile_regex(grammar)
    raise ValueError(f"grammar: a ByteDFA, a BytePDA or a pattern string (got {type(grammar).__name__})")


class TokenBytes:
    """Every token's byte string, flat: ``off`` (N + 1,) int32, ``bytes`` (off[N],) uint8; token i is ``bytes[off[i] : off[i + 1]]``."""

    def __init__(self, off, data):
        self.off = np.ascontiguousarray(off, dtype=np.int32)
        self.bytes = np.ascontiguousarray(data, dtype=np.uint8)
        if self.off.ndim != 1 or self.off.size < 2 or self.off[0] != 0 or np.any(np.diff(self.off) < 0) or self.off[-1] != self.bytes.size:
            raise ValueError("TokenBytes: off must rise from 0 to len(bytes) over N + 1 >= 2 entries")

    def __len__(self):
        return self.off.size - 1

    def token(self, i: int) -> bytes:
        return self.bytes[self.off[i]:self.off[i + 1]].tobytes()

    def tokens(self):
        return [self.token(i) for i in range(len(self))]

    def join(self, ids) -> bytes:
        """The bytes a sequence of ids stands for - what a grammar constrains.  Ids outside the table count as empty.  (sentencepiece's
        own ``decode`` additionally drops ONE leading space, the dummy prefix its encoder puts in front of a text.)"""
        n = len(self)
        return b"".join(self.token(int(i)) for i in ids if 0 <= int(i) < n)

    def padded(self, n: int) -> "TokenBytes":
        """The table extended with empty tokens to ``n`` entries (a model's padded vocabulary)."""
        if n < len(self):
            raise ValueError(f"TokenBytes.padded: {len(self)} tokens do not fit {n}")
        if n == len(self):
            return self
        return TokenBytes(np.concatenate([self.off, np.full(n - len(self), self.off[-1], dtype=np.int32)]), self.bytes)


def token_byte_table(source) -> TokenBytes:
    """``source``: a list of ``bytes`` - taken as given - or a tokenizer that names its sentencepiece file (``decoder.SentencePieceIds``, the
    reference's tokenizer object: ``decoder.tok_file_of``).  From a sentencepiece vocabulary: a piece with "▁" replaced by a space,
    UTF-8 encoded; a byte-fallback piece ``<0xNN>`` is that one byte; control, unknown and unused pieces and the five special tokens
    behind the sentencepiece vocabulary are EMPTY (a grammar never allows an empty token)."""
    if isinstance(source, TokenBytes):
        return source
    if isinstance(source, (list, tuple)):
        if any(not isinstance(t, (bytes, bytearray)) for t in source):
            raise ValueError("token_byte_table: a list of bytes objects")
        toks = [bytes(t) for t in source]
    else:
        from .decoder import SentencePieceIds, tok_file_of
        sp = getattr(source, "sp", None) if isinstance(source, SentencePieceIds) else None
        if sp is None:
            f = tok_file_of(source)
            if f is None:
                raise ValueError(f"token_byte_table: {type(source).__name__} names no sentencepiece file (pass a list of bytes)")
            import sentencepiece
            sp = sentencepiece.SentencePieceProcessor(model_file=str(f))
        toks = []
        for i in range(len(sp)):
            if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i):
                toks.append(b"")
            elif sp.is_byte(i):
                toks.append(bytes([int(sp.id_to_piece(i)[3:5], 16)]))
            else:
                toks.append(sp.id_to_piece(i).replace("▁", " ").encode("utf-8"))
        toks += [b""] * len(SentencePieceIds.SPECIAL)
    off = np.zeros(len(toks) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in toks], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("token_byte_table: the vocabulary's bytes do not fit int32 offsets")
    return TokenBytes(off.astype(np.int32), np.frombuffer(b"".join(toks), dtype=np.uint8))
