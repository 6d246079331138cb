// verify_tree — is TREE the elimination tree of GRAPH's records under SEQ?  (No reference
// analogue: the check graph2tree -c means to make, for a .tre from any source — a -l part and
// merge_trees, a multi-rank run, another build.)
//
//   verify_tree GRAPH SEQ TREE [-l n/k] [-v]
//
// GRAPH loads as partition_tree -g loads it (-l n/k: only part n of k, for a part's own
// tree); SEQ "-" is the degree sequence of the loaded records.  Prints "Tree is valid." or
// "ERROR: Tree is not valid." and one line with the four counts and the first offender of
// each class (sheep_verify_t; "-" where there is none).  Exit status: 0 valid, 2 not valid,
// 1 usage or I/O errors.
#include <unistd.h>

#include <chrono>

#include "sheep/sheep.hpp"

using namespace sheep;

static bool readable(const char *name) {
  FILE *f = fopen(name, "rb");
  if (f) fclose(f);
  return f != nullptr;
}

// "n/k" with 1 <= n <= k, nothing else in the string
static bool parse_part(const char *s, size_t *part, size_t *num_parts) {
  char *end = nullptr;
  if (*s < '0' || *s > '9') return false;
  const unsigned long long n = strtoull(s, &end, 10);
  if (*end != '/' || end[1] < '0' || end[1] > '9') return false;
  const unsigned long long k = strtoull(end + 1, &end, 10);
  if (*end != '\0' || n < 1 || n > k) return false;
  *part = (size_t)n;
  *num_parts = (size_t)k;
  return true;
}

static void print_count(const char *label, uint64_t count, uint64_t first, const char *sep) {
  if (first == UINT64_MAX) printf("%s:%zu@-%s", label, (size_t)count, sep);
  else printf("%s:%zu@%zu%s", label, (size_t)count, (size_t)first, sep);
}

int main(int argc, char *argv[]) {
  size_t part = 0, num_parts = 0;
  bool verbose = false;
  opterr = 0;
  int opt;
  while ((opt = getopt(argc, argv, "l:v")) != -1) {
    switch (opt) {
      case 'l':
        if (!parse_part(optarg, &part, &num_parts)) {
          printf("Option -l requires n/k with 1 <= n <= k.\n");
          return 1;
        }
        break;
      case 'v': verbose = !verbose; break;
      case '?':
        if (optopt == 'l') printf("Option -%c requires a string.\n", optopt);
        else printf("Unknown option character '\\x%x'.\n", optopt);
        return 1;
      default: abort();
    }
  }
  if (optind + 3 != argc) {
    printf("USAGE: verify_tree input_graph input_sequence input_tree [-l n/k] [-v]\n");
    return 1;
  }
  const char *graph_filename = argv[optind], *sequence_filename = argv[optind + 1], *tree_filename = argv[optind + 2];
  const bool degree_seq = strcmp(sequence_filename, "-") == 0;
  for (const char *name : {graph_filename, degree_seq ? graph_filename : sequence_filename, tree_filename})
    if (!readable(name)) {
      printf("verify_tree: cannot read %s\n", name);
      return 1;
    }

  try {
    auto start_point = std::chrono::steady_clock::now();
    auto seconds = [&]() {
      return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start_point).count() /
             1000.0;
    };
    JNodeTable jnodes(tree_filename);
    GraphWrapper graph(graph_filename, part, num_parts);
    DeviceSequence seq = degree_seq ? degreeSequence(graph) : uploadSequence(readSequence(sequence_filename));
    if (verbose) printf("Loaded in: %f seconds\n", seconds());
    sheep_verify_t v;
    const bool ok = JTree::isValid(jnodes, graph, seq, &v);
    if (verbose) printf("Verified in: %f seconds\n", seconds());
    if (ok) {
      printf("Tree is valid.\n");
      return 0;
    }
    printf("ERROR: Tree is not valid.\n");
    if (jnodes.size() != seq.n) {
      printf("nodes:%zu sequence:%zu\n", (size_t)jnodes.size(), (size_t)seq.n);
    } else {
      print_count("bad_parent", v.bad_parent, v.first_bad_parent, " ");
      print_count("not_descendant", v.not_descendant, v.first_not_descendant, " ");
      print_count("unsupported", v.unsupported, v.first_unsupported, " ");
      print_count("pst_mismatch", v.pst_mismatch, v.first_pst_mismatch, "\n");
    }
    return 2;
  } catch (const std::out_of_range &e) {
    fprintf(stderr, "verify_tree: %s\n", e.what());   // a neighbour beyond the sequence's largest vid
    return 1;
  } catch (const std::bad_alloc &) {
    fprintf(stderr, "verify_tree: cannot load the inputs (std::bad_alloc)\n");
    return 1;
  } catch (const std::exception &e) {
    fprintf(stderr, "verify_tree: %s\n", e.what());
    return 1;
  }
}
