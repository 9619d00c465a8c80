####################################################################################################
# Result tables of a test pass of the model-free path on MI355X (reference: report_phoneme_to_articulation.py:128-296):
# results_dir/test_outputs/0/<sentence>/ -> tract_variables.csv, error_report_full.csv, error_report_agg.csv and
# TV_corr_report.csv under results_dir.
#
#   python report_phoneme_to_articulation.py --config configs/report_synthetic.yaml
#
# The YAML keys are the keyword arguments of main(), the reference's.  The per-sentence plots of the reference are not
# produced.  run_test, run_transformer_test and the mean-contour test write the same four files at the end of their own
# pass with `report_dir=`, without reading anything back.
####################################################################################################
import argparse

import yaml

from artspeech_amd.phoneme_to_articulation.report import report_from_results_dir


def main(database_name, results_dir, articulators):
    paths = report_from_results_dir(database_name, results_dir, articulators).write(results_dir)
    for path in paths.values():
        print(path)
    return paths


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    args = parser.parse_args()
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    main(**cfg)
