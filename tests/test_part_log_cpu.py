"""Host side of the partitioned arrival log (gs_run_partitioned_log): the symbol in the
library, the header, the ctypes table and the integration notes; the ABI number stays."""
import inspect
import os
import re

import gossipsim

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAME = "gs_run_partitioned_log"


def test_symbol_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    assert hasattr(gossipsim.lib(), NAME)
    assert NAME + "(" in header
    res, args = gossipsim.SIGNATURES[NAME]
    assert len(args) == 8 and args[5] is gossipsim.TEXT_FN
    decl = header[header.index("gs_status " + NAME + "("):]
    assert decl[:decl.index(";")].count(",") == 7  # the same eight arguments
    assert re.search(r"#define\s+GS_ABI_VERSION\s+10u?\s", header)


def test_bindings_and_documents():
    fn = gossipsim.Comm.run_partitioned_log
    assert callable(fn)
    assert list(inspect.signature(fn).parameters)[1:] == ["sims", "schedule", "on_text", "paths", "chunk_bytes"]
    par = inspect.signature(gossipsim.Comm.run_partitioned).parameters
    assert "on_lat" in par and "block_msgs" in par
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = open(os.path.join(ROOT, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    assert "pub fn " + NAME + "(" in rust
