#!/usr/bin/env python3
"""Writes tests/golden/imageclassify_merge.csv: what pandas' `pd.merge(df, df_results).to_csv()` gives on the fixture of
tests/imageclassify_fixture.py (duplicate and missing case numbers, a quoted prompt with a comma, float32 scores with 1.0,
a denormal and a 9-digit value).  test_imageclassify_host.py compares SD/eval-scripts/imageclassify.py's own writer with
these bytes, and with pandas where pandas is installed.  Needs pandas; run from the repository root."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> int:
    import imageclassify_fixture as X
    path = os.path.join(ROOT, "tests", "golden", "imageclassify_merge.csv")
    data = X.merge_with_pandas()
    with open(path, "wb") as f:
        f.write(data)
    print(f"{path}: {len(data)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
