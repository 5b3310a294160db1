"""Hand-written kernels in llvm-objdump's format, for the tests of the build rules under tools/ (they read text, so a
fragment of a few hundred lines stands in for a kernel): one writer for every test that needs one."""

NAME = "_ZN12_GLOBAL__N_111k_step_imu9IdfLi8ELb1EEEvN7kfpos_k5KArgsE"
NAME_P48 = "_ZN12_GLOBAL__N_111k_step_imu9IN7kfpos_k3p48EfLi8ELb1EEEvNS1_5KArgsE"
KERNEL = (r"k_step_imu9IdfLi8ELb1E",)
FMA = "v_fma_f64 v[4:5], v[0:1], v[0:1], v[4:5]"


class Fragment:
    """One function: emit() appends instructions, label() names the next one, branch() appends a branch to a label
    (set before or after); text() renders it, four bytes an instruction, branch targets as objdump prints them."""

    def __init__(self, name=NAME, base=0x1000):
        self.name, self.base, self.body, self.labels, self.fix = name, base, [], {}, {}

    def emit(self, *ins):
        self.body.extend(ins)

    def label(self, name):
        self.labels[name] = len(self.body)

    def branch(self, op, name):
        self.fix[len(self.body)] = name
        self.body.append(op)

    def text(self):
        lines = [f"{self.base:016x} <{self.name}>:"]
        for i, ins in enumerate(self.body):
            tail = ""
            if i in self.fix:
                target = self.labels[self.fix[i]]
                ins += f" {(target - i - 1) % 65536}"
                tail = f" <{self.name}+{4 * target:#x}>"
            lines.append(f"\t{ins}  // {self.base + 4 * i:012X}: BF800000{tail}")
        return "\n".join(lines) + "\n"
