"""CPU: static check of the handle-lifetime guard of the C ABI (csrc/engine.hpp `Guard`) and of the threading sentence the two documents carry.

include/gpmi355.h and INTEGRATION.md promise that every function taking a handle may be called from any OS thread and is serialised per ctx; engine.hpp
promises that such a call cannot race a concurrent *_free / gp_ctx_destroy: the handle is pinned under the registry mutex, the ctx is locked, and the handle
is checked again under the lock.  That only holds if EVERY exported entry point whose first parameter is a gp_ctx*, gp_post* or gp_vfe* starts with the
Guard — one function added without it is a use-after-free under threads that no single-threaded test sees.  Here the `extern "C"` definitions of
gpmi355.hip, batch.hip and multi.hip are parsed against the header:

  - the first statement that touches the handle constructs a `Guard` on it and the next one is the `!gd.ok` return, or
  - it hands the handle to ONE shared body (`return body(handle, ...)`: batch_impl, the *_any templates, the dev_* templates) that starts that way, or
  - it is one of the three releasing functions, which take the handle out of the registry (`reg_take`) BEFORE they lock the ctx.

tests/test_gpu_threads.py is the dynamic side (two to four host threads on real contexts)."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "abstractgps.jl_amd" / "csrc"
HEADER = ROOT / "include" / "gpmi355.h"
UNITS = ("gpmi355.hip", "batch.hip", "multi.hip")
HANDLES = {"gp_ctx": "not a live gp_ctx", "gp_post": "not a live gp_post", "gp_vfe": "not a live gp_vfe"}
RELEASING = {"gp_ctx_destroy": "gp_ctx", "gp_posterior_free": "gp_post", "gp_vfe_free": "gp_vfe"}


def strip_comments(txt: str) -> str:
    """C / C++ comments replaced by blanks, string literals kept (the "not a live ..." texts are checked)."""
    out, i, n = [], 0, len(txt)
    while i < n:
        c = txt[i]
        if c == '"':
            j = i + 1
            while j < n and txt[j] != '"':
                j += 2 if txt[j] == "\\" else 1
            out.append(txt[i:j + 1])
            i = j + 1
        elif txt.startswith("//", i):
            j = txt.find("\n", i)
            i = n if j < 0 else j
        elif txt.startswith("/*", i):
            j = txt.find("*/", i + 2)
            out.append(" ")
            i = n if j < 0 else j + 2
        else:
            out.append(c)
            i += 1
    return "".join(out)


def _close(s: str, i: int, open_ch: str, close_ch: str) -> int:
    """index of the bracket that closes the one at s[i] (string literals skipped)"""
    depth, j, n = 0, i, len(s)
    while j < n:
        ch = s[j]
        if ch == '"':
            j += 1
            while s[j] != '"':
                j += 2 if s[j] == "\\" else 1
        elif ch == open_ch:
            depth += 1
        elif ch == close_ch:
            depth -= 1
            if depth == 0:
                return j
        j += 1
    raise ValueError("unbalanced " + open_ch)


def statements(body: str) -> list:
    """the top-level statements of a function body: split at ';' outside every bracket; a braced block ends a statement too"""
    out, cur, depth, j, n = [], "", 0, 0, len(body)
    while j < n:
        ch = body[j]
        if ch == '"':
            k = j + 1
            while body[k] != '"':
                k += 2 if body[k] == "\\" else 1
            cur += body[j:k + 1]
            j = k + 1
            continue
        if ch in "({[":
            depth += 1
        elif ch in ")}]":
            depth -= 1
        cur += ch
        if depth == 0 and (ch == ";" or ch == "}"):
            if cur.strip():
                out.append(" ".join(cur.split()))
            cur = ""
        j += 1
    if cur.strip():
        out.append(" ".join(cur.split()))
    return out


def header_handle_functions(header_text: str) -> dict:
    """name -> handle type, for every declared gp_* / gpd_* function whose FIRST parameter is a gp_ctx*, gp_post* or gp_vfe* (not a gp_ctx**)"""
    txt = strip_comments(header_text)
    out = {}
    for m in re.finditer(r"\b(?:int32_t|int64_t)\s+(gpd?_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        first = m.group(2).split(",")[0]
        h = re.fullmatch(r"\s*(gp_ctx|gp_post|gp_vfe)\s*\*\s*[A-Za-z_]\w*\s*", first)
        if h:
            out[m.group(1)] = h.group(1)
    return out


def definitions(src: str) -> dict:
    """name -> (first parameter's name, body) of every function DEFINED in the (comment-free) source text whose return type is int32_t / int64_t"""
    out = {}
    for m in re.finditer(r"\b(?:int32_t|int64_t)\s+([A-Za-z_]\w*)\s*\(", src):
        lp = m.end() - 1
        rp = _close(src, lp, "(", ")")
        k = rp + 1
        while k < len(src) and src[k].isspace():
            k += 1
        if k >= len(src) or src[k] != "{":
            continue  # a declaration or a call
        rb = _close(src, k, "{", "}")
        first = src[lp + 1:rp].split(",")[0]
        pm = re.search(r"([A-Za-z_]\w*)\s*$", first)
        out.setdefault(m.group(1), (pm.group(1) if pm else "", src[k + 1:rb]))
    return out


def exported_definitions(src: str) -> set:
    """the gp_* / gpd_* functions a translation unit defines with C linkage: inside an `extern "C" { ... }` block (nested `extern "C++"` blocks excluded)
    or with an `extern "C"` prefix of their own"""
    names = set(re.findall(r'extern\s+"C"\s+(?:int32_t|int64_t|const\s+char\s*\*)\s*(gpd?_[a-z0-9_]+)\s*\(', src))
    for m in re.finditer(r'extern\s+"C"\s*\{', src):
        lb = m.end() - 1
        block = src[lb + 1:_close(src, lb, "{", "}")]
        while True:  # cut the extern "C++" islands (templates shared by the wrappers)
            mm = re.search(r'extern\s+"C\+\+"\s*\{', block)
            if not mm:
                break
            block = block[:mm.start()] + block[_close(block, mm.end() - 1, "{", "}") + 1:]
        depth = 0
        for line_m in re.finditer(r"[{}]|\b(?:int32_t|int64_t|const\s+char\s*\*)\s*(gpd?_[a-z0-9_]+)\s*\(", block):
            tok = line_m.group(0)
            if tok == "{":
                depth += 1
            elif tok == "}":
                depth -= 1
            elif depth == 0:
                names.add(line_m.group(1))
    return names


def guard_problem(name: str, handle: str, defs: dict, _depth: int = 0):
    """None when `name` starts with the guard on its handle (directly or through one shared body), else the reason it does not"""
    if name not in defs:
        return f"{name}: no definition found"
    h, body = defs[name]
    st = statements(body)
    uses = [i for i, s in enumerate(st) if re.search(rf"\b{re.escape(h)}\b", s)]
    if not uses:
        return f"{name}: never touches its handle `{h}`"
    i = uses[0]
    g = re.fullmatch(rf"Guard (\w+)\({re.escape(h)}(?:, (?:true|false))?\);", st[i])
    if g:
        nxt = st[i + 1] if i + 1 < len(st) else ""
        if not re.match(rf"if \(!{g.group(1)}\.ok\) return\b", nxt):
            return f"{name}: the statement after the Guard is not the `!{g.group(1)}.ok` return: `{nxt}`"
        if "not a live" in nxt and HANDLES[handle] not in nxt:
            return f"{name}: the dead-handle text is not \"{HANDLES[handle]}\": `{nxt}`"
        return None
    d = re.fullmatch(rf"return (\w+)(?:<[^<>]*>)?\({re.escape(h)}\b.*\);", st[i])
    if d and _depth < 2 and d.group(1) in defs and not re.match(r"gpd?_", d.group(1)):
        p = guard_problem(d.group(1), handle, defs, _depth + 1)
        return p and f"{name}: through its body {p}"
    return f"{name}: the first statement that touches `{h}` is neither a Guard on it nor a call of a guarded body: `{st[i]}`"


def release_problem(name: str, handle: str, defs: dict):
    if name not in defs:
        return f"{name}: no definition found"
    h, body = defs[name]
    st = statements(body)
    if not st or not re.match(rf"if \(!{h} \|\| !reg_take\({h}\)\) return\b", st[0]) or HANDLES[handle] not in st[0]:
        return f"{name}: does not start by taking `{h}` out of the registry: `{st[0] if st else ''}`"
    take, lock = body.find("reg_take("), body.find("->mu")
    if lock < 0:
        return f"{name}: never takes the ctx lock (a call still using the handle would not be waited for)"
    if not take < lock:
        return f"{name}: locks the ctx before reg_take"
    if "Guard" in body:
        return f"{name}: a releasing function must not construct a Guard (it would pin the handle it is about to delete)"
    return None


def check_sources(header_text: str, sources: dict) -> list:
    """every finding over the given header / {unit: source text}; [] = the contract holds"""
    want = header_handle_functions(header_text)
    clean = {u: strip_comments(t) for u, t in sources.items()}
    defs, exported = {}, set()
    for u in clean:
        for k, v in definitions(clean[u]).items():
            defs.setdefault(k, v)
        exported |= exported_definitions(clean[u])
    declared = set(re.findall(r"\b(gpd?_[a-z0-9_]+)\s*\(", strip_comments(header_text)))
    problems = [f"{n}: defined with C linkage but not declared in include/gpmi355.h" for n in sorted(exported - declared)]
    problems += [f"{n}: declared in the header but not defined with C linkage" for n in sorted(set(want) - exported)]
    for name, handle in sorted(want.items()):
        p = release_problem(name, handle, defs) if name in RELEASING else guard_problem(name, handle, defs)
        if p:
            problems.append(p)
    return problems


def _sources() -> dict:
    return {u: (CSRC / u).read_text() for u in UNITS}


def test_the_header_lists_the_handle_functions_this_check_is_about():
    want = header_handle_functions(HEADER.read_text())
    assert len(want) >= 60, len(want)  # 63 at the time of writing: a parser that silently finds a handful would pass everything
    assert {"gp_logpdf": "gp_ctx", "gp_logpdf_batch": "gp_ctx", "gpd_sync": "gp_ctx", "gpd_gemm_nt_f32": "gp_ctx", "gp_ctx_multi_info": "gp_ctx",
            "gp_posterior_predict": "gp_post", "gp_posterior_n": "gp_post", "gp_vfe_grad": "gp_vfe", "gp_vfe_m": "gp_vfe"}.items() <= want.items()
    assert RELEASING.items() <= want.items()
    assert "gp_ctx_create" not in want and "gp_last_error" not in want and "gp_rccl_selftest" not in want


def test_every_handle_entry_point_starts_with_the_guard():
    problems = check_sources(HEADER.read_text(), _sources())
    assert not problems, "\n".join(problems)


def test_the_guard_itself_pins_locks_and_rechecks():
    """The three steps engine.hpp documents, in that order, and the registry removal the re-check relies on."""
    eng = strip_comments((CSRC / "engine.hpp").read_text())
    i = eng.index("struct Guard {")
    g = eng[i:_close(eng, eng.index("{", i), "{", "}")]
    pin, lock, recheck = g.index("lock_guard<std::mutex> l(g_reg_mu)"), g.index("unique_lock<std::mutex>(c->mu)"), g.index("reg_has((void*)h) && !c->dead")
    assert pin < g.index("g_live.count((void*)h)") < g.index("c->refs++") < lock < recheck
    assert "ctx_unref(c)" in g[g.index("~Guard()"):]
    src = strip_comments((CSRC / "gpmi355.hip").read_text())
    assert re.search(r"static\s+thread_local\s+std::string\s+g_err\s*;", src), "gp_last_error()'s text is documented as thread-local"


@pytest.mark.parametrize("mutation", ["guard_line_deleted", "ok_return_deleted", "guard_after_use", "unguarded_function_added", "free_locks_before_reg_take",
                                      "wrapper_body_unguarded"])
def test_the_check_fails_on_an_unguarded_entry_point(mutation):
    """The parser is only worth something if it refuses the sources it exists to refuse: each mutation edits the TEXT (nothing is compiled or run)."""
    hdr, src = HEADER.read_text(), _sources()
    g = src["gpmi355.hip"]
    if mutation == "guard_line_deleted":
        a = g.index("int32_t gp_posterior_solve(")
        g = g[:a] + g[a:].replace("    Guard gd(post);\n", "", 1)
        expect = "gp_posterior_solve"
    elif mutation == "ok_return_deleted":
        a = g.index("int32_t gp_ctx_trim(")
        g = g[:a] + g[a:].replace('    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");\n', "", 1)
        expect = "gp_ctx_trim"
    elif mutation == "guard_after_use":
        a = g.index("int32_t gp_get_timings(")
        g = g[:a] + g[a:].replace("    Guard gd(c);\n", "    const int dev = c->device;\n    Guard gd(c);\n", 1)
        expect = "gp_get_timings"
    elif mutation == "unguarded_function_added":
        hdr = hdr.replace("int32_t gp_ctx_trim(gp_ctx* ctx);", "int32_t gp_ctx_trim(gp_ctx* ctx);\nint32_t gp_ctx_peek(gp_ctx* ctx, int64_t* out);")
        g = g.replace("int32_t gp_ctx_trim(gp_ctx* c) {", "int32_t gp_ctx_peek(gp_ctx* c, int64_t* out) {\n    *out = (int64_t)c->pool.size();\n    return 0;\n}\n\nint32_t gp_ctx_trim(gp_ctx* c) {")
        expect = "gp_ctx_peek"
    elif mutation == "free_locks_before_reg_take":
        a = g.index("int32_t gp_vfe_free(")
        g = g[:a] + g[a:].replace('    if (!p || !reg_take(p)) return set_arg_err(1, "not a live gp_vfe");\n',
                                  '    std::lock_guard<std::mutex> l0(p->ctx->mu);\n    if (!p || !reg_take(p)) return set_arg_err(1, "not a live gp_vfe");\n', 1)
        expect = "gp_vfe_free"
    else:
        b = src["batch.hip"]
        assert "    Guard gd(c);\n" in b
        src["batch.hip"] = b.replace("    Guard gd(c);\n", "", 1)
        expect = "gp_logpdf_batch"
    assert g != _sources()["gpmi355.hip"] or mutation == "wrapper_body_unguarded"
    src["gpmi355.hip"] = g
    problems = check_sources(hdr, src)
    assert any(p.startswith(expect) for p in problems), (mutation, problems)
    if mutation != "wrapper_body_unguarded":
        assert len(problems) == 1, problems
    else:
        assert sorted(p.split(":")[0] for p in problems) == ["gp_logpdf_batch", "gp_logpdf_batch_sum"], problems


def _threading_claims(text: str) -> dict:
    t = " ".join(re.sub(r"[`*]", "", text).split()).lower()
    return {"any_thread": bool(re.search(r"may (?:be called|come) from any (?:os|julia) thread", t)),
            "serialised_per_ctx": bool(re.search(r"serialised (?:per ctx )?by an internal mutex", t)) and ("per ctx" in t or "on one gp_ctx" in t),
            "thread_local_error": bool(re.search(r"gp_last_error\(\) \(thread-local\)|thread-local gp_last_error\(\)", t))}


def test_header_and_integration_md_make_the_same_threading_promise():
    hdr = HEADER.read_text()
    conv = hdr[hdr.index("Conventions"):hdr.index("#ifndef GPMI355_H")]
    integ = (ROOT / "INTEGRATION.md").read_text()
    para = integ[integ.index("Conventions the shim relies on"):integ.index("## 3.")]
    h, i = _threading_claims(conv.replace(" * ", " ").replace("\n *", "\n")), _threading_claims(para)
    assert h == {"any_thread": True, "serialised_per_ctx": True, "thread_local_error": True}, h
    assert i == h, (i, h)
