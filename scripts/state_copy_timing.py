"""Time the state save / load / fork kernels against a plain device-to-device copy of the same number of bytes.

    python scripts/state_copy_timing.py [--num-envs 4096 65536] [--launches 100] [--out FILE]

Per case: HIP events around blocks of 20 back-to-back launches, alternating with blocks of 20 `copy_` launches of a float32 tensor
with as many bytes as the case moves one way (record_words * 4 * lanes), after a warm-up block of each; the mean per launch of
both and their ratio are printed as one JSON line per case.  The figures in DESIGN.md ("Measurements: state save / load / fork")
come from this script."""
import query_timing as qt
import torch

BLOCK = 20


def measure(fn, base, launches):
    """query_timing.measure with the blocks of `fn` and of `base` alternating, so that both see the same session: (us, base us)."""
    fn(); base()
    qt.time_block(fn, BLOCK); qt.time_block(base, BLOCK)           # warm-up
    tf = tb = 0.0
    blocks = max(1, (launches + BLOCK - 1) // BLOCK)
    for _ in range(blocks):
        tf += qt.time_block(fn, BLOCK)
        tb += qt.time_block(base, BLOCK)
    return tf / (blocks * BLOCK), tb / (blocks * BLOCK)


def main():
    args = qt.parser(launches=100, num_envs=[4096, 65536]).parse_args()
    dev = qt.DEV
    lines = []
    for n in args.num_envs:
        core = qt.blind_grasping_core(n)
        _, words = core.state_layout()
        bank = core.state_bank(core.NS)
        core.save_state(bank)
        g = torch.Generator(device=dev).manual_seed(0)
        half = torch.arange(n // 2, device=dev)
        rnd = torch.randperm(n, device=dev, generator=g)[:256]
        slots = torch.arange(256, device=dev)
        small = core.state_bank(256)
        ones = torch.zeros(n - 1, dtype=torch.int64, device=dev)
        rest = torch.arange(1, n, device=dev)
        cases = [
            ("full save", core.NS, lambda: core.save_state(bank)),
            ("full load", core.NS, lambda: core.load_state(bank)),
            ("copy_envs wg-to-wg, first half of the envs onto the second", n // 2, lambda: core.copy_envs(half, half + n // 2)),
            ("copy_envs env 0 into all others", n - 1, lambda: core.copy_envs(ones, rest)),
            ("save 256 random ids", 256, lambda: core.save_state(small, env_ids=rnd, slots=slots)),
            ("load 256 random ids", 256, lambda: core.load_state(small, env_ids=rnd, slots=slots)),
        ]
        for name, lanes, fn in cases:
            nbytes = words * 4 * lanes
            src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
            dst = torch.empty_like(src)
            us, base_us = measure(fn, lambda: dst.copy_(src), args.launches)
            line = {"num_envs": n, "case": name, "lanes": lanes, "MB": round(nbytes / 1e6, 2), "us": round(us, 1),
                    "copy_us": round(base_us, 1), "ratio": round(us / base_us, 2), "GBps_one_way": round(nbytes / us / 1e3, 1)}
            qt.emit(line)
            lines.append(line)
            del src, dst
        core.close()
        del core, bank, small
        torch.cuda.empty_cache()
    qt.write(args, lines)


if __name__ == "__main__":
    main()
