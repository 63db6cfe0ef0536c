"""The pipelined convolution's instantiation table (conv_pipe.hip build_rows) as the library lists it -- fc_debug_conv_table_read, host
code, no device -- against the symbol table of the gfx950 code objects in the built library (tools/flavour_sizes.py: symbol sizes only)
and against the allow-list of the ledger in tests/test_gpu_conv_table.py.  No GPU needed.

  * the hook returns 197 distinct rows, with the length and truncation behaviour of fc_debug_conv_routes_read;
  * the rows are exactly the conv_pipe_kernel instantiations the code object holds: one compiled but not in the table could never be
    launched through it, one in the table but not compiled could not have linked -- either way the two lists must not drift;
  * every row the ledger allows without a numerical gate is a row of the table;
  * every row with phase stamps (FL_STAMP) has an unstamped twin -- the same arguments with the bit cleared -- which is what the
    ledger compares it with, bit for bit.
"""
import ctypes as C

from conv_table_rows import ALLOW, FL_STAMP, A_FL

N_ROWS = 197
# stamped rows the table deliberately has no unstamped twin for (none today)
STAMPED_WITHOUT_TWIN = set()


def table_rows():
    from flocoder_amd import _binding as B
    lib = B.lib()
    n = lib.fc_debug_conv_table_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    assert lib.fc_debug_conv_table_read(buf, n + 1) == n
    text = buf.value.decode()
    assert len(text) == n and text.endswith("\n")
    return [tuple(int(v) for v in line.split()) for line in text.splitlines()]


def test_the_hook_lists_197_distinct_rows_of_thirteen_arguments():
    rows = table_rows()
    assert len(rows) == N_ROWS and len(set(rows)) == N_ROWS
    assert all(len(r) == 13 for r in rows)
    assert table_rows() == rows                      # a second listing is the same: nothing accumulates between calls


def test_the_hook_counts_and_truncates_like_the_route_record():
    from flocoder_amd import _binding as B
    lib = B.lib()
    n = lib.fc_debug_conv_table_read(None, 0)
    full = C.create_string_buffer(n + 1)
    lib.fc_debug_conv_table_read(full, n + 1)
    for cap in (1, 2, 10, n, n + 1, n + 50):
        buf = C.create_string_buffer(b"\xff" * (cap + 4), cap + 4)
        assert lib.fc_debug_conv_table_read(buf, cap) == n             # always the full length
        keep = min(n, cap - 1)
        assert buf.raw[:keep] == full.raw[:keep] and buf.raw[keep] == 0      # truncated to cap - 1 bytes and NUL-terminated
        assert buf.raw[cap:cap + 4] == b"\xff" * 4                           # nothing written past cap
    assert lib.fc_debug_conv_table_read(full, 0) == n and lib.fc_debug_conv_table_read(None, 64) == n


def test_the_table_equals_the_code_objects_symbol_table():
    from flocoder_amd import _binding as B
    from tools.flavour_sizes import kernel_sizes
    compiled = set(kernel_sizes(B.LIB_PATH))
    table = set(table_rows())
    assert table - compiled == set(), f"rows without device code: {sorted(table - compiled)}"
    assert compiled - table == set(), f"compiled instantiations no launch can reach: {sorted(compiled - table)}"


def test_every_allowed_row_is_a_row_of_the_table():
    table = set(table_rows())
    assert len(ALLOW) <= 20
    assert set(ALLOW) <= table, f"stale allow-list entries: {sorted(set(ALLOW) - table)}"
    assert all(isinstance(v, str) and len(v) > 40 for v in ALLOW.values())       # each with its reason


def test_every_stamped_row_has_an_unstamped_twin():
    table = set(table_rows())
    stamped = {r for r in table if r[A_FL] != 4095 and (r[A_FL] & FL_STAMP)}
    assert len(stamped) == 58
    orphans = {r for r in stamped if r[:A_FL] + (r[A_FL] & ~FL_STAMP,) + r[A_FL + 1:] not in table}
    assert orphans == STAMPED_WITHOUT_TWIN, sorted(orphans ^ STAMPED_WITHOUT_TWIN)
