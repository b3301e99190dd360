"""WeightAlign's MI355X half without a GPU: the tiling choice and the weight stream built by
csrc/stream_builder.cpp are walked by a CPU emulation of the tiled kernel's dataflow
(tests/cpp/emulate_tiled.cpp: LDS planes, lane->quad mapping, bucket walk, accumulator classes,
shift-and-sum epilogue) and compared with a plain dense convolution on 35 geometries; the same for
the machine code csrc/jit_codegen.cpp generates, run by an interpreter of its instruction forms -- unit by
unit, and as whole-tile chains (waits, barriers, buffer rotation in code) where the generator chains them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_and_self_initialising_code_against_cpu_emulation(tmp_path):
    """The LDS-staged stream and the generated code of 44 geometries, emulated instruction by instruction against a
    dense convolution.  Generated code always initialises its own accumulators (jit_codegen.h): every case must."""
    exe = str(tmp_path / "emulate_tiled")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "emulate_tiled.cpp"),
                           os.path.join(csrc, "align_rules.cpp"), os.path.join(csrc, "stream_builder.cpp"), os.path.join(csrc, "jit_codegen.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert "all cases OK" in text
    # 44 geometries (five of them on four-wave workgroups by hand; the last four take the generated code's tiling and options
    # from the product's layout rule, align_rules.h) through the LDS-staged weight stream and again through the code jit_codegen.cpp
    # generates, interpreted instruction by instruction
    assert text.count("rel_err=") == 44 + 44
    assert len([l for l in text.splitlines() if l.startswith("jit ")]) == 44
    # ... every one of them with code that initialises its own accumulators (first products as multiplies, the quads block 0
    # never touches cleared at its top; the interpreter starts those accumulators as NaN and refuses an FMA onto one)
    init = [tuple(int(v) for v in l.split("init=")[1].split()[0].split("+")) for l in text.splitlines() if l.startswith("jit ")]
    assert sum(1 for m, z in init if m > 0) >= 20 and sum(1 for m, z in init if z > 0) >= 3
    assert all(m + z > 0 for m, z in init), init
    # ... a good part of them as chains (one call per tile), several blocks long, with one and two fills in flight
    chained = [l for l in text.splitlines() if l.startswith("jit chained ")]
    assert len(chained) >= 15
    assert sum(1 for l in chained if int(l.split("icb=")[1].split()[0].split("/")[1]) >= 3) >= 4


def test_stream_loop_generator_reads_no_environment():
    """gen_stream_loop.py writes the same stream_loop_asm.inc whatever the build shell holds: the ESC_GEN_* variables it
    once read (priorities, store modifiers, an alignment pass) cannot change the product kernel."""
    import sys
    gen = os.path.join(ROOT, "caffe-escoin_amd", "csrc", "gen_stream_loop.py")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ESC_GEN_")}
    want = subprocess.run([sys.executable, gen], env=clean, stdout=subprocess.PIPE, check=True, timeout=300).stdout
    dirty = dict(clean, ESC_GEN_NOPRIO="1", ESC_GEN_STORE_MOD=" nt", ESC_GEN_ALIGN="4", ESC_GEN_PRIO_QUADS="0",
                 ESC_GEN_PRIO_HI="2", ESC_GEN_PRIO_YOUNG="0", ESC_GEN_PRIO_YOUNG_HI="1")
    got = subprocess.run([sys.executable, gen], env=dirty, stdout=subprocess.PIPE, check=True, timeout=300).stdout
    assert len(want) > 100000 and b"ESC2_LOOP_ASM_BAND_YOUNG_DMA" in want
    assert got == want


def test_channel_deal_is_a_permutation_and_never_worse(tmp_path):
    """balance_channels (WeightAlign): slot -> channel table is a permutation; the modelled cost of
    the slowest wave per block, summed, does not exceed the natural order's (tests/cpp/balance_check.cpp)."""
    exe = str(tmp_path / "balance_check")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "balance_check.cpp"),
                           os.path.join(csrc, "stream_builder.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert "all cases OK" in text
    # ... and the tables are pinned: the deal is deterministic (seeded patterns, hashes of the slot -> channel tables).
    # Round 5 changed where the refinement starts (a global longest-processing-time-first deal instead of the natural
    # order: stream_builder.cpp), hence new hashes; the incremental cost update itself was pinned against the
    # recompute-everything version in round 4.
    assert re.findall(r"table ([0-9a-f]{16})", text) == [
        "0f1fec86ccd5a1e5", "8cc9987d3bd9de89", "7dfc8de268d31c5d", "de43a4a92d53df97", "7e6a10f6a0edf747", "b73140c29c11e44f",
        "1f054c7da250324f"]
