#!/usr/bin/env python
"""tests/golden/nt_tasks.json: the Nucleotide Transformer benchmark's task table, parsed from the
reference's configs/dataset/nucleotide_transformer.yaml -- every top-level entry that is a
mapping with train_len, classes, max_length and metric (the per-task entries its interpolations
`${.${.dataset_name}.max_length}` ... read). Settings only; finetune_data.NT_TASKS restates it and
tests/test_nt_host.py compares the two.

    DNA_REFERENCE=<reference checkout> python tests/golden/make_nt_tasks.py
"""
import json
import os

import yaml

REF = os.environ.get("DNA_REFERENCE", "/root/reference")
FIELDS = ("train_len", "classes", "max_length", "metric")


def main():
    with open(os.path.join(REF, "configs", "dataset", "nucleotide_transformer.yaml")) as f:
        data = yaml.safe_load(f)
    tasks = {name: {k: entry[k] for k in FIELDS} for name, entry in data.items()
             if isinstance(entry, dict) and all(k in entry for k in FIELDS)}
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nt_tasks.json")
    with open(out, "w") as f:
        json.dump(tasks, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(tasks)} tasks")


if __name__ == "__main__":
    main()
