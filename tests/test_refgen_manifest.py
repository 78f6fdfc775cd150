"""CPU: `tools/refgen` (the Rust program that runs the REFERENCE and writes tests/golden/ref_*; it cannot be compiled in
this image) stays one command away from working -- its manifest is checked against the reference's (VERDICT r5 item 7;
the round-5 slip was a missing `loader_halo2`, which gates `system::halo2::transcript::halo2::PoseidonTranscript`):
  * every Cargo feature it asks of `snark-verifier` exists there, and every module its `use snark_verifier::{...}` tree
    names is enabled by one of them (`#[cfg(feature = "...")] pub mod x;` in the reference's module tree);
  * halo2curves / halo2_proofs resolve to the version / tag the reference pins;
  * the extractor that wrote the fixture these checks read (tests/golden/gen_reference_manifest.py ->
    tests/golden/reference_manifest.json) reads back exactly that fixture from a crate laid out as it describes."""
import json
import os
import re

import tomli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFGEN = os.path.join(ROOT, "tools", "refgen")


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "reference_manifest.json")) as f:
        return json.load(f)


def _use_paths(src, crate):
    """every `crate::a::b::Leaf` path of the `use crate::{...};` trees in `src`, flattened"""
    out = []

    def expand(prefix, body):
        depth, start, items = 0, 0, []
        for i, ch in enumerate(body):
            if ch == "{":
                depth += 1
            elif ch == "}":
                depth -= 1
            elif ch == "," and depth == 0:
                items.append(body[start:i])
                start = i + 1
        items.append(body[start:])
        for it in items:
            it = it.strip()
            if not it:
                continue
            m = re.match(r"^([\w:]+?)::\{(.*)\}$", it, re.S)
            if m:
                expand(prefix + m.group(1).split("::"), m.group(2))
            else:
                out.append(prefix + it.split(" as ")[0].strip().split("::"))

    for m in re.finditer(r"use %s::(\{.*?\}|[\w:]+);" % crate, src, re.S):
        body = m.group(1)
        expand([], body[1:-1] if body.startswith("{") else body)
    return out


def test_refgen_features_enable_every_module_it_uses():
    fx = _fixture()
    man = tomli.load(open(os.path.join(REFGEN, "Cargo.toml"), "rb"))
    dep = man["dependencies"]["snark-verifier"]
    assert dep.get("default-features") is False  # explicit features: a changed default must not go unnoticed
    feats = set(dep["features"])
    assert feats <= set(fx["features"]), feats - set(fx["features"])
    src = open(os.path.join(REFGEN, "src", "main.rs")).read()
    paths = _use_paths(src, "snark_verifier")
    assert len(paths) >= 15 and ["system", "halo2", "transcript", "halo2", "PoseidonTranscript"] in paths
    needed = {}
    for p in paths:
        for k in range(1, len(p) + 1):
            gate = fx["module_gates"].get("::".join(p[:k]))
            if gate:
                needed.setdefault(gate, "::".join(p))
    assert needed, "the gate table matched nothing: the fixture or the parser is broken"
    missing = {g: via for g, via in needed.items() if g not in feats}
    assert not missing, "tools/refgen/Cargo.toml lacks feature(s) %s" % missing
    # serialising `Snark` / `PlonkProtocol` (bincode / serde_json in main.rs) needs the reference's serde derives
    if "bincode::" in src or "serde_json::to" in src:
        assert "derive_serde" in feats


def test_refgen_resolves_the_dependency_versions_the_reference_pins():
    fx = _fixture()
    deps = tomli.load(open(os.path.join(REFGEN, "Cargo.toml"), "rb"))["dependencies"]
    assert deps["halo2curves"]["version"] == fx["halo2curves_version"] == "0.6.0"  # the arithmetic under test
    assert deps["halo2_proofs"]["git"] == fx["halo2_proofs_git"] and deps["halo2_proofs"]["tag"] == fx["halo2_proofs_tag"]
    assert "github.com/privacy-scaling-explorations/snark-verifier" in deps["snark-verifier"]["git"]


def _write_crate(crate, fx):
    """a miniature `snark-verifier` crate with the fixture's manifest entries and module tree: every gated module under its
    `#[cfg(feature = "...")]`, every module on the way to one declared plainly, src/a/b.rs for `a::b`"""
    toml = ['[package]', 'name = "snark-verifier"', 'version = "%s"' % fx["crate_version"], "", "[features]"]
    toml += ["%s = [%s]" % (k, ", ".join('"%s"' % d for d in v)) for k, v in sorted(fx["feature_deps"].items())]
    toml += ["", "[dependencies]", 'halo2_curves = { version = "%s", package = "halo2curves" }' % fx["halo2curves_version"],
             'halo2_proofs = { git = "%s", tag = "%s", optional = true }' % (fx["halo2_proofs_git"], fx["halo2_proofs_tag"])]
    os.makedirs(os.path.join(crate, "src"))
    with open(os.path.join(crate, "Cargo.toml"), "w") as f:
        f.write("\n".join(toml) + "\n")
    children = {}
    for path in fx["module_gates"]:
        parts = path.split("::")
        for k in range(1, len(parts) + 1):
            children.setdefault(tuple(parts[:k - 1]), set()).add(parts[k - 1])
    for parent, names in children.items():
        rs = os.path.join(crate, "src", *parent) + ".rs" if parent else os.path.join(crate, "src", "lib.rs")
        os.makedirs(os.path.dirname(rs), exist_ok=True)
        with open(rs, "w") as f:
            for name in sorted(names):
                gate = fx["module_gates"].get("::".join(parent + (name,)))
                f.write(('#[cfg(feature = "%s")]\n' % gate if gate else "") + "pub mod %s;\n" % name)


def test_the_manifest_extractor_reproduces_the_fixture(tmp_path):
    import importlib.util

    fx = _fixture()
    crate = os.path.join(str(tmp_path), "snark-verifier")
    _write_crate(crate, fx)
    spec = importlib.util.spec_from_file_location("_genman", os.path.join(ROOT, "tests", "golden", "gen_reference_manifest.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    g.CRATE = crate
    assert g.extract() == fx
