// big_puzzle.hpp -- the library's own Puzzle of up to 25 cells as a device environment (BigPuzzleEnv: the big_* functions the Puzzle
// kernels call, as a struct) built as a module: the tests drive its host side against the oracle's Puzzle and its kernels against tw.env.Puzzle's.
#pragma once
#include "twisterl_device_env.hpp"
#include "tw_big_board.hpp"
using BigPuzzle25 = tw::BigPuzzleEnv<25>;
