// cli_args_main.cpp — csrc/host/cli_args.h alone, for tests/test_cli_args.py and tests/test_sanitizers.py: every line of stdin is one
// command line, its arguments after argv[0] separated by tabs (an empty line: no arguments; an empty field: an empty argument).  Per
// line one line of stdout: `usage`, or `accept <mode>`.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../rust-raytracer_amd/csrc/host/cli_args.h"

int main() {
  static const char* const mode_name[] = {"usage", "one-shot", "progressive", "denoised-one-shot", "adaptive", "animation", "denoised-animation"};  // cli::Mode
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> args{"raytracer"};
    if (!line.empty()) {
      size_t at = 0;
      for (size_t tab; (tab = line.find('\t', at)) != std::string::npos; at = tab + 1) args.push_back(line.substr(at, tab - at));
      args.push_back(line.substr(at));
    }
    std::vector<char*> argv;
    for (std::string& a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    const cli::Options o = cli::parse((int)args.size(), argv.data());
    if (o.mode == cli::USAGE) std::puts("usage");
    else std::printf("accept %s\n", mode_name[o.mode]);
  }
  return 0;
}
