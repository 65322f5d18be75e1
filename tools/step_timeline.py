"""The last step of a bench.py run as a kernel timeline, from a rocprofv3 kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o b -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras
    python tools/step_timeline.py DIR/.../b_kernel_trace.csv
One line per kernel of the step (the launches between the last two decode kernels): name, start ms, end ms, duration ms,
grid -- the format of profiles/r3_folder_timeline.txt."""
import csv
import sys

SHORT = {"frame_yin_kernel": "frame", "pyin_obs_kernel": "obs", "db_rake_kernel": "db_rake", "rake_pow_kernel": "rake_pow",
         "rake_runs_kernel": "rake_runs", "decode_kernel": "decode"}


def main(path):
    rows = [r for r in csv.DictReader(open(path)) if "aegis::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dec = [i for i, r in enumerate(rows) if "decode_kernel" in r["Kernel_Name"]]
    step = rows[(dec[-2] + 1 if len(dec) > 1 else 0):dec[-1] + 1]
    t0 = int(step[0]["Start_Timestamp"])
    for r in step:
        name = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("aegis::", "")
        if name == "chunk_signal_kernel":
            continue
        name = SHORT.get(name, "viterbi" if "viterbi" in name else name)
        s, e = (int(r["Start_Timestamp"]) - t0) / 1e6, (int(r["End_Timestamp"]) - t0) / 1e6
        print(f"{name:12s} {s:8.2f} {e:8.2f} {e - s:7.2f} {r.get('Grid_Size') or r.get('Grid_Size_X', '')}")


if __name__ == "__main__":
    main(sys.argv[1])
