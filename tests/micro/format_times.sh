#!/bin/sh
# tests/micro/format_times.py on the parent commit's build and on this one, interleaved, three runs in one session:
#   sh tests/micro/format_times.sh PARENT_TREE        (a built checkout of the parent commit: its package and its library)
# Every GPU step runs under a time limit of its own, and its exit status is checked: the first step that fails, faults or runs
# into its limit ends the script with that status, and nothing more is started on the GPU.
parent=${1:?usage: format_times.sh PARENT_TREE}
here=$(dirname "$0")
for run in 1 2 3; do
  timeout -k 10 120 python "$here/format_times.py" --tree "$parent" --formats s16 --tag "run $run parent" || exit $?
  timeout -k 10 240 python "$here/format_times.py" --tag "run $run this build" || exit $?
done
