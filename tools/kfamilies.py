"""Per-setup kernel-family sums of rocprofv3 --stats kernel_stats.csv files, side by side:
python tools/kfamilies.py <setups in each run> <csv> [<csv> ...]
Families: the radix sort, the transpose fill and helpers, the row merges (mpm), the
point-wise products, the map copies, device-to-device copies; everything else as 'other'."""
import csv
import sys

FAMILIES = [("radix_sort_onesweep", "radix_sort_onesweep"), ("radix_sort other", "radix_sort"),
            ("k_tr_fill", "k_tr_fill"), ("k_row_of_entry", "k_row_of_entry"), ("k_iota", "k_iota"),
            ("k_ro_from_sorted/gaps", "k_ro_"), ("k_mpm_wave", "k_mpm_wave"), ("k_mpm_flag", "k_mpm_flag"),
            ("k_mpm", "k_mpm<"), ("k_pointwise_sum", "k_pointwise_sum"), ("k_pointwise", "k_pointwise"),
            ("k_perm_vals", "k_perm_vals"), ("k_rows_strict", "k_rows_strict"),
            ("copyBuffer", "copyBuffer"), ("k_diag*", "k_diag"),
            ("k_qfactor_blk 64", "k_qfactor_blk<64,"), ("k_qfactor_blk 128", "k_qfactor_blk<128,"),
            ("k_qfactor_blk 256", "k_qfactor_blk<256,"), ("k_qfactor_blk 512", "k_qfactor_blk<512,"),
            ("k_qfactor_blk 1024", "k_qfactor_blk<1024,")]


def sums(path, setups):
    out = {name: [0, 0.0] for name, _ in FAMILIES}
    out["other"] = [0, 0.0]
    for r in csv.DictReader(open(path)):
        for name, key in FAMILIES:
            if key in r["Name"]:
                break
        else:
            name = "other"
        out[name][0] += int(r["Calls"])
        out[name][1] += float(r["TotalDurationNs"]) / 1e6 / setups
    out["all kernels"] = [sum(v[0] for v in out.values()), sum(v[1] for v in out.values())]
    return out


def main():
    setups = int(sys.argv[1])
    cols = [sums(p, setups) for p in sys.argv[2:]]
    print("family (ms per setup; calls in the run)".ljust(40) + "".join(p[-40:].rjust(44) for p in sys.argv[2:]))
    for name in list(cols[0]):
        print(name.ljust(40) + "".join(f"{c[name][1]:12.1f} ms {c[name][0]:8d} calls".rjust(44) for c in cols))


if __name__ == "__main__":
    main()
