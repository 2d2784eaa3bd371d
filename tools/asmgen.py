"""What more than one of the asm generators needs (gen_fp_chain_asm.py, gen_f6_asm.py, gen_jac_asm.py, isa_probe/gen.py):
the entry wait of a statement, what an instruction line reads and writes, the wait-state padding, and the text of one
SSA_DEV function around one asm statement.  Nothing here knows a field, a curve or a register assignment."""
import re

# First instruction of every statement.  The compiler keeps values in registers these statements clobber and reloads them from
# scratch behind each statement; it waits for such a reload where the VALUE is next used -- not in front of an inline asm
# that merely clobbers the register (measured: ssa_k_sign entered the gathering addition with four reloads in flight, which
# then landed in the statement's temporaries: wrong signatures on ~7 % of the waves, different ones from run to run).  The
# statements whose operands the compiler loads itself were shielded by its wait for those operands; the gathering ones are
# not.  So: nothing of the compiler's may be in flight when a statement starts.
ENTRY_WAIT = "s_waitcnt vmcnt(0)"

# mnemonics with two destinations: the result, then the carry-out (an SGPR pair or VCC)
TWO_DST = frozenset(("v_mad_u64_u32", "v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32", "v_subbrev_co_u32"))


def _regs(operand):
    m = re.match(r"v\[(\d+):(\d+)\]$", operand)
    if m:
        return [("v", r) for r in range(int(m.group(1)), int(m.group(2)) + 1)]
    m = re.match(r"v(\d+)$", operand)
    if m:
        return [("v", int(m.group(1)))]
    m = re.match(r"s\[(\d+):\d+\]$", operand)
    if m:
        return [("s", int(m.group(1)))]
    return [("s", "vcc")] if operand == "vcc" else []


def reads_writes(line):
    """(registers read, registers written) of one instruction line, by operand position: ("v", n) a VGPR, ("s", n) the SGPR
    pair s[n:n+1], ("s", "vcc").  Constants and %[name] operands of the statement count as nothing."""
    mnem, _, rest = line.partition(" ")
    ops = [o.strip() for o in rest.split(",")]
    n_dst = 2 if mnem in TWO_DST else 1
    return [r for o in ops[n_dst:] for r in _regs(o)], [r for o in ops[:n_dst] for r in _regs(o)]


def pad_wait_states(lines, gap=3):
    """insert s_nop so that a VALU read of an SGPR pair / VCC comes at least `gap` positions after its VALU write"""
    out, written = [], {}
    for ln in lines:
        if ln.startswith("v_"):
            rd, wr = reads_writes(ln)
            need = max([gap - (len(out) - written[r]) for r in rd if r in written] + [0])
            if need > 0:
                out.append("s_nop %d" % (need - 1))
                # an s_nop N occupies one position and N + 1 wait states: account for it as `need` positions
                for k in written:
                    written[k] -= need - 1
            for r in wr:
                if r[0] == "s":
                    written[r] = len(out)
        out.append(ln)
    return out


def asm_lines(body):
    """the instruction lines as the quoted lines of an asm statement"""
    return ['        "%s%s"' % (ln, "\\n\\t" if i + 1 < len(body) else "") for i, ln in enumerate(body)]


def clobbers(vgprs, sgprs, extras):
    """the clobber list: VGPR numbers, SGPR numbers (an int n: s0 .. s(n-1)), then names such as "vcc", "scc", "memory" """
    sgprs = range(sgprs) if isinstance(sgprs, int) else sgprs
    return ['"v%d"' % r for r in vgprs] + ['"s%d"' % r for r in sgprs] + ['"%s"' % e for e in extras]


def pinned(regs, name, mode="+"):
    """the operands name[0..] pinned to the register pairs regs (mode "+": in and out, "": input)"""
    return ['"%s{v[%d:%d]}"(%s[%d])' % (mode, r, r + 1, name, j) for j, r in enumerate(regs)]


def statement(doc, signature, body, outputs, inputs, clobber, volatile=False, before=(), after=()):
    """the lines of the SSA_DEV function `signature` that is one asm statement: doc = comment lines, before / after = C lines
    around the statement, outputs / inputs = operand rows (one source line each; an empty list leaves the section empty)"""
    def section(rows):
        return "        : " + ",\n          ".join(rows) if rows else "        :"
    return ["// " + d for d in doc] + ["SSA_DEV %s {" % signature] + ["    " + c for c in before] + \
        ["    asm volatile(" if volatile else "    asm("] + asm_lines(body) + [section(outputs), section(inputs)] + \
        ["        : " + ", ".join(clobber) + ");"] + ["    " + c for c in after] + ["}"]
