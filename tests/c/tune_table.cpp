// The switch table of ckb_zkp_amd/csrc/tune.hpp, stand-alone (host compiler, no GPU, nothing else of the library):
//     tune_table [NAME=value ...]
// clears every ZKP_* variable it inherited, sets the ones given, and prints what a context created now would latch
// (tune_dump: NAME=value, one line per row).  tests/test_tune_table.py holds the expected values.
#include <cstring>
#include <string>
#include <vector>

#include "tune.hpp"

extern char** environ;

int main(int argc, char** argv) {
  std::vector<std::string> inherited;
  for (char** e = environ; *e; e++)
    if (!strncmp(*e, "ZKP_", 4)) inherited.emplace_back(*e, strcspn(*e, "="));
  for (const std::string& name : inherited) unsetenv(name.c_str());
  for (int i = 1; i < argc; i++) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return 2;
    setenv(std::string(argv[i], eq - argv[i]).c_str(), eq + 1, 1);
  }
  zkp::tune_dump(zkp::tune_from_env(), stdout);
  return 0;
}
