"""The reference-side binding a maintainer applies (integration/*.patch) must apply to the pristine reference tree.

Self-contained: tests/golden/reference_patch_targets.json pins the four pristine files the patches edit -- line counts, the
SHA-256 of every region a hunk replaces and how often the strings below occur -- and none of their text enters the
repository (tests/golden/make_patch_fixture.py writes it from a reference checkout).
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = ["lib_rs.patch", "group_rs.patch", "pcdl_rs.patch", "acc_rs.patch"]
# what the checks below count in the patched files (single-line strings: a patch changes a file line by line)
NEEDLES = ["mod ffi;", "ffi::", "crate::ffi::", "msm_unchecked", "ffi::KEY as GS", "ipa.round_lr(&H_prime)", "gs[j + m]",
           "crate::ffi::h_accumulate(h_0, &xis, alphas)", "crate::ffi::h_eval_batch(&xis, z)", "self.hs[i].get_poly()",
           "self.hs[i].eval(z)", "let mut h = PallasPoly::zero();"]


def parse_patch(text):
    """one-file unified diff -> (path, hunks); every hunk's line counts must agree with its header"""
    lines = text.splitlines(keepends=True)
    assert lines[0].startswith("--- a/") and lines[1].startswith("+++ b/"), lines[:2]
    rel = lines[0][6:].rstrip("\n")
    assert lines[1][6:].rstrip("\n") == rel
    hunks, i = [], 2
    while i < len(lines):
        m = re.fullmatch(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@.*\n", lines[i])
        assert m, "not a hunk header: %r" % lines[i]
        h = {"old_start": int(m.group(1)), "old_len": int(m.group(2) or 1), "new_start": int(m.group(3)), "new_len": int(m.group(4) or 1),
             "old": [], "new": [], "minus": [], "plus": []}
        i += 1
        into = {" ": ("old", "new"), "-": ("old", "minus"), "+": ("new", "plus")}
        prev = ()
        while i < len(lines) and not lines[i].startswith("@@ "):
            tag, body = lines[i][0], lines[i][1:]
            if tag == "\\":  # "\ No newline at end of file": the line before it has none
                for k in prev:
                    h[k][-1] = h[k][-1].rstrip("\n")
            else:
                assert tag in into, "bad line in a hunk: %r" % lines[i]
                prev = into[tag]
                for k in prev:
                    h[k].append(body)
            i += 1
        assert (len(h["old"]), len(h["new"])) == (h["old_len"], h["new_len"]), "hunk header of %s at -%d disagrees with its body" % (rel, h["old_start"])
        hunks.append(h)
    assert hunks
    return rel, hunks


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "reference_patch_targets.json")) as f:
        return json.load(f)["files"]


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def _write_stand_in(dest):
    """A stand-in of the pristine tree: every region a hunk replaces as the patch states it, every other line a placeholder."""
    fx = _fixture()
    for name in PATCHES:
        rel, hunks = parse_patch(open(os.path.join(ROOT, "integration", name)).read())
        f = fx[rel]
        lines = ["// line %d of the pristine file (not stored here)\n" % (k + 1) for k in range(f["lines"])]
        for h in hunks:
            lines[h["old_start"] - 1: h["old_start"] - 1 + h["old_len"]] = h["old"]
        assert len(lines) == f["lines"]
        if not f["ends_with_newline"]:
            lines[-1] = lines[-1].rstrip("\n")
        path = os.path.join(dest, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as out:
            out.write("".join(lines))


def test_patches_apply_to_the_pristine_reference():
    """Every hunk replaces, at the line it names, exactly the pristine lines (their SHA-256 is pinned), so `patch -p1` applies
    each patch without offset or fuzz; the patched files then contain the calls and none of the replaced bodies."""
    fx = _fixture()
    after, added = {}, {}
    for name in PATCHES:
        rel, hunks = parse_patch(open(os.path.join(ROOT, "integration", name)).read())
        f = fx[rel]
        assert [(h["old_start"], h["old_len"]) for h in hunks] == [(x["old_start"], x["old_len"]) for x in f["hunks"]], name
        end, shift = 0, 0
        for h, x in zip(hunks, f["hunks"]):
            assert h["old_start"] > end, "%s: hunks overlap or are out of order" % name
            end = h["old_start"] + h["old_len"] - 1
            assert end <= f["lines"], "%s: hunk at -%d runs past the end of the pristine file" % (name, h["old_start"])
            assert h["new_start"] == h["old_start"] + shift, "%s: hunk at -%d has the wrong new start" % (name, h["old_start"])
            shift += h["new_len"] - h["old_len"]
            assert _sha("".join(h["old"])) == x["sha256"], "%s: the lines the hunk at -%d replaces are not the pristine ones" % (name, h["old_start"])
        # the patched file's count of each string: the pristine count, less what the hunks remove, plus what they add
        after[os.path.basename(rel)] = {s: f["counts"][s] - sum(l.count(s) for h in hunks for l in h["minus"])
                                        + sum(l.count(s) for h in hunks for l in h["plus"]) for s in NEEDLES}
        assert f["counts"]["ffi::"] == 0, rel  # every ffi:: of a patched file comes from the patch
        added[os.path.basename(rel)] = "".join(l for h in hunks for l in h["plus"])
    group, pcdl, lib, acc = after["group.rs"], after["pcdl.rs"], after["lib.rs"], after["acc.rs"]
    assert lib["mod ffi;"] >= 1
    assert group["msm_unchecked"] == 0 and group["crate::ffi::"] == 4
    assert pcdl["ffi::KEY as GS"] >= 1 and pcdl["ipa.round_lr(&H_prime)"] >= 1 and pcdl["gs[j + m]"] == 0
    # a13: AccumulatedHPolys::get_poly / eval (acc.rs:85-106) go to halo_h_accumulate / halo_h_eval_batch
    assert acc["crate::ffi::h_accumulate(h_0, &xis, alphas)"] >= 1 and acc["crate::ffi::h_eval_batch(&xis, z)"] >= 1
    assert acc["self.hs[i].get_poly()"] == 0 and acc["self.hs[i].eval(z)"] == 0 and acc["let mut h = PallasPoly::zero();"] == 0
    # every ffi:: function a patched file calls exists in ffi.rs
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    defined = set(re.findall(r"pub fn (\w+)\s*[(<]", ffi)) | {"KEY", "Ipa"}
    for text in (added["group.rs"], added["pcdl.rs"], added["acc.rs"]):
        for name in re.findall(r"crate::ffi::(\w+)", text) + re.findall(r"ffi::(KEY)", text):
            assert name in defined, name


def test_patches_are_what_make_patches_writes(tmp_path):
    """The committed patches are the generator's output (no hand edits: that is how a hunk header went wrong before).  The
    generator runs on the stand-in of the pristine tree, whose replaced regions the test above pins by hash."""
    before = {n: open(os.path.join(ROOT, "integration", n)).read() for n in PATCHES}
    ref = tmp_path / "reference"
    _write_stand_in(str(ref))
    out = tmp_path / "integration"
    shutil.copytree(os.path.join(ROOT, "integration"), out)
    subprocess.run([sys.executable, str(out / "make_patches.py")], check=True, capture_output=True, env=dict(os.environ, HALO_REFERENCE=str(ref)))
    for n in PATCHES:
        assert (out / n).read_text() == before[n], n


def _strip_rust(src):
    """comments and string / char literals blanked (same length), so that brackets inside them do not count"""
    import re
    out = re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), src)
    out = re.sub(r'"(?:[^"\\\n]|\\.)*"', lambda m: '"' + " " * (len(m.group(0)) - 2) + '"', out)
    out = re.sub(r"'(?:[^'\\\n]|\\.)'", lambda m: "' '".ljust(len(m.group(0))), out)
    return out


def _split_args(arglist):
    """top-level comma split of a parameter list"""
    args, depth, cur = [], 0, ""
    for ch in arglist:
        if ch in "(<[":
            depth += 1
        elif ch in ")>]":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        args.append(cur.strip())
    return args


def _c_class(param):
    """coarse class of a C parameter: ptr / fn / usize / int / u64"""
    p = param.strip()
    if "halo_allgather_fn" in p:
        return "fn"
    if "*" in p or "[" in p:
        return "ptr"
    for key, cls in (("size_t", "usize"), ("uint64_t", "u64"), ("int", "int")):
        if key in p.split():
            return cls
    raise AssertionError("unclassified C parameter: %r" % param)


def _rust_class(param):
    ty = param.split(":", 1)[1].strip()
    if ty.startswith("*"):
        return "ptr"
    return {"usize": "usize", "c_int": "int", "u64": "u64", "HaloAllgatherFn": "fn"}[ty]


def _c_class_rccl(param):
    p = param.strip()
    if "*" in p or "[" in p:
        return "ptr"
    return "usize" if "size_t" in p.split() else "int"


def _header_prototypes(name="halo_accumulation.h"):
    import re
    header = open(os.path.join(ROOT, "include", name)).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b([A-Za-z_][\w \*]*?)\b(halo_\w+)\s*\(([^;{}]*?)\)\s*;", header):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "typedef" in ret:
            continue
        params = [] if args in ("", "void") else _split_args(args)
        protos[name] = (ret, params)
    return protos


def test_ffi_rs_is_structurally_sound():
    """integration/ffi.rs is never compiled here (no Rust toolchain), and it has been wrong before: a `#[link]` attribute
    that ended up on a type alias.  This is a structural lint, not a compiler: every `#[link` sits
    directly on an `extern "C" {` block, brackets balance, every item of the extern block is a `pub fn ...;`, and every
    declaration has the arity, the parameter classes (pointer / usize / c_int / u64 / callback) and the return class of the
    prototype in include/halo_accumulation.h."""
    import re
    raw = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    src = _strip_rust(raw)
    # 1. brackets balance (and never go negative)
    pairs = {")": "(", "]": "[", "}": "{"}
    stack = []
    for i, ch in enumerate(src):
        if ch in "([{":
            stack.append((ch, i))
        elif ch in ")]}":
            assert stack and stack[-1][0] == pairs[ch], "unbalanced %r at offset %d (line %d)" % (ch, i, src.count("\n", 0, i) + 1)
            stack.pop()
    assert not stack, "unclosed %r at line %d" % (stack[-1][0], src.count("\n", 0, stack[-1][1]) + 1)
    # 2. every #[link ...] attribute is followed (attributes / blank lines aside) by `extern "C" {`, and every extern block has one
    links = [m.end() for m in re.finditer(r"#\[link\s*\([^\]]*\)\]", src)]
    assert links, "no #[link] attribute"
    for end in links:
        rest = src[end:].lstrip()
        while rest.startswith("#["):
            rest = rest[rest.index("]") + 1:].lstrip()
        assert re.match(r'extern\s+"\s*"\s*\{', rest), "#[link] does not decorate an extern block: %r" % rest[:60]  # (literals are blanked)
    blocks = list(re.finditer(r'extern\s+"[^"]*"\s*\{', src))
    assert len(blocks) == len(links) == 1
    assert re.search(r'#\[link\s*\(\s*name\s*=\s*"halo_hip"\s*\)\]\s*extern\s+"C"\s*\{', raw), "the extern block lost its #[link(name = \"halo_hip\")]"
    # 3. the extern block: only `pub fn name(args) [-> ret];` items
    start = blocks[0].end()
    depth, i = 1, start
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    body = src[start:i - 1]
    items = [it.strip() for it in body.split(";")]
    assert items[-1] == "", "the last item of the extern block does not end in ';'"
    decls = {}
    for it in items[:-1]:
        m = re.fullmatch(r"pub fn (halo_\w+)\s*\((.*)\)\s*(?:->\s*(.+))?", it, flags=re.S)
        assert m, "not a `pub fn ...;` declaration: %r" % it[:80]
        assert m.group(1) not in decls, "declared twice: " + m.group(1)
        decls[m.group(1)] = (_split_args(m.group(2)), (m.group(3) or "").strip())
    # 4. against the header: arity, parameter classes, return class
    protos = _header_prototypes()
    assert len(protos) > 80
    for name, (params, ret) in decls.items():
        assert name in protos, name + " is not declared in the header"
        c_ret, c_params = protos[name]
        assert len(params) == len(c_params), "%s: %d parameters in ffi.rs, %d in the header" % (name, len(params), len(c_params))
        for k, (rp, cp) in enumerate(zip(params, c_params)):
            assert re.match(r"\w+\s*:", rp), "%s: parameter %d has no name: %r" % (name, k, rp)
            assert _rust_class(rp) == _c_class(cp), "%s: parameter %d is %r in ffi.rs and %r in the header" % (name, k, rp, cp)
        want = "ptr" if "*" in c_ret else "void" if c_ret.split()[-1] == "void" else "int" if c_ret.split()[-1] == "int" else "usize"
        got = "ptr" if ret.startswith("*") else "void" if ret == "" else {"c_int": "int", "usize": "usize"}[ret]
        assert got == want, "%s: returns %r in ffi.rs, %r in the header" % (name, ret, c_ret)
    # 5. every halo_* function the wrappers call is declared in the extern block
    called = set(re.findall(r"\b(halo_\w+)\s*\(", src[i:]))
    assert called <= set(decls), sorted(called - set(decls))
    # 6. what the patches need is there: the a13 binding and the multi-device context
    for need in ("halo_h_accumulate", "halo_h_eval_batch", "halo_ctx_create_multi"):
        assert need in decls and need in called, need
    assert "HALO_DEVICES" in raw and "dyn PrimeField" not in raw


def test_ffi_rccl_rs_matches_its_header():
    """integration/ffi_rccl.rs (the optional RCCL all-gather for a Rust host) against include/halo_rccl.h: brackets
    balance, #[link(name = "halo_rccl")] sits on the one extern block, every declaration has the header's arity, parameter
    classes and return class, and every header symbol is declared."""
    import re
    raw = open(os.path.join(ROOT, "integration", "ffi_rccl.rs")).read()
    src = _strip_rust(raw)
    pairs, stack = {")": "(", "]": "[", "}": "{"}, []
    for i, ch in enumerate(src):
        if ch in "([{":
            stack.append(ch)
        elif ch in ")]}":
            assert stack and stack.pop() == pairs[ch], "unbalanced %r at line %d" % (ch, src.count("\n", 0, i) + 1)
    assert not stack
    assert re.search(r'#\[link\s*\(\s*name\s*=\s*"halo_rccl"\s*\)\]\s*extern\s+"C"\s*\{', raw)
    blocks = list(re.finditer(r'extern\s+"[^"]*"\s*\{', src))
    assert len(blocks) == 1
    start = blocks[0].end()
    depth, i = 1, start
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    items = [it.strip() for it in src[start:i - 1].split(";")]
    assert items[-1] == ""
    protos = _header_prototypes("halo_rccl.h")
    decls = {}
    for it in items[:-1]:
        m = re.fullmatch(r"pub fn (halo_\w+)\s*\((.*)\)\s*(?:->\s*(.+))?", it, flags=re.S)
        assert m, it[:80]
        decls[m.group(1)] = (_split_args(m.group(2)), (m.group(3) or "").strip())
    assert set(decls) == set(protos), (sorted(set(protos) - set(decls)), sorted(set(decls) - set(protos)))
    for name, (params, ret) in decls.items():
        c_ret, c_params = protos[name]
        assert len(params) == len(c_params), name
        for rp, cp in zip(params, c_params):
            ty = rp.split(":", 1)[1].strip()
            got = "ptr" if ty.startswith("*") else {"usize": "usize", "c_int": "int"}[ty]
            assert got == _c_class_rccl(cp), (name, rp, cp)
        want = "ptr" if "*" in c_ret else "void" if c_ret.split()[-1] == "void" else "int" if c_ret.split()[-1] == "int" else "usize"
        got = "ptr" if ret.startswith("*") else "void" if ret == "" else {"c_int": "int", "usize": "usize"}[ret]
        assert got == want, (name, ret, c_ret)
    # the callback it hands out has the type the core shim's sharded entry points take
    assert "crate::ffi::HaloAllgatherFn { Some(halo_allgather_rccl) }" in raw
    assert "pub type HaloAllgatherFn = Option<unsafe extern \"C\" fn(user: *mut c_void, send: *const u64, words: usize, recv: *mut u64) -> c_int>;" in open(os.path.join(ROOT, "integration", "ffi.rs")).read()


def test_shim_declares_only_exported_symbols():
    """every `pub fn halo_*` of ffi.rs is declared in the header (the link step of a cargo build would fail otherwise)"""
    import re
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    names = set(re.findall(r"pub fn (halo_\w+)\(", ffi))
    assert names and all(re.search(r"\b%s\(" % n, header) for n in names), sorted(n for n in names if not re.search(r"\b%s\(" % n, header))


def test_integration_md_quotes_ffi_rs_verbatim():
    """the declarations INTEGRATION.md section 1 shows are the lines of integration/ffi.rs (no second, drifting copy)"""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    quoted = [l for l in md.splitlines() if l.strip().startswith("pub fn halo_")]
    assert len(quoted) >= 20
    for l in quoted:
        assert l.strip() in ffi, l
    assert '#[link(name = "halo_hip")]\nextern "C" {' in md
